"""KeccakGoldilocksConfig (plonk/config.rs:110-118: Hasher = KeccakHash<25>, InnerHasher = PoseidonHash): Keccak-256 Merkle trees,
transcript and proof of work.

PARITY UNPINNED against Rust: the reference holds no Keccak known-answer vector and there is no Rust toolchain, so what stands in for the
oracle is the independent model in THIS file -- a numpy Keccak-f[1600] sponge (round constants from the LFSR, rotation offsets from the
(x, y) walk: no table shared with csrc/keccak.cuh), checked against hashlib.sha3_256 and the two published Keccak-256 digests, and on top
of it hash_or_noop, two_to_one, hash_pad, Merkle trees, KeccakPermutation and (over the duplex model of tests/transcript.py) a Challenger restated from the reference's sources."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle_lib import P, rand_field
from proof_parser import NUM_WIRES, ParsedProof, leaf_lens, opening_columns
from transcript import DuplexChallenger, LibraryChallenger, drive_phase_api, public_inputs_hash, replay_transcript

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
KECCAK = "keccak"


# ------------------------------------------------------------------------------------------------------ the model: Keccak-f[1600]
def _round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) % 256
            if r & 2:
                rc ^= 1 << ((1 << j) - 1)
        out.append(rc)
    return out


def _rotation_offsets():
    rot = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        rot[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC, ROT = _round_constants(), _rotation_offsets()


def _rotl(v, r):
    return v if r == 0 else (v << U64(r)) | (v >> U64(64 - r))


def keccak_f(states):
    """Keccak-f[1600] on [n][25] uint64 states (lane x + 5 y), vectorised over n."""
    a = [states[:, i].copy() for i in range(25)]
    for rnd in range(24):
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x - 1) % 5] ^ _rotl(c[(x + 1) % 5], 1) for x in range(5)]
        b = [None] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y] ^ d[x], ROT[x][y])
        for y in range(5):
            for x in range(5):
                a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y])
        a[0] = a[0] ^ U64(RC[rnd])
    return np.stack(a, axis=1)


def sponge256(msgs, domain):
    """[n][L] uint8 messages of one length -> [n][32] uint8: rate 136, capacity 512, pad = domain byte ... 0x80."""
    msgs = np.asarray(msgs, dtype=np.uint8).reshape(len(msgs), -1)
    n, length = msgs.shape
    pad = np.zeros((n, 136 - length % 136), dtype=np.uint8)
    pad[:, 0] ^= domain
    pad[:, -1] ^= 0x80
    full = np.ascontiguousarray(np.concatenate([msgs, pad], axis=1))
    s = np.zeros((n, 25), dtype=U64)
    for blk in range(full.shape[1] // 136):
        s[:, :17] ^= np.ascontiguousarray(full[:, 136 * blk:136 * (blk + 1)]).view("<u8")
        s = keccak_f(s)
    return np.ascontiguousarray(s[:, :4]).view(np.uint8)


def keccak256(msgs):
    return sponge256(msgs, 0x01)


def test_model_is_sha3_with_domain_06_and_keccak256_with_domain_01():
    # C1: the sponge with a selectable domain byte; block boundaries at 135 / 136 / 137 bytes
    for length in (0, 3, 135, 136, 137, 1080):
        m = bytes((7 * i + length) % 256 for i in range(length))
        assert sponge256(np.frombuffer(m, dtype=np.uint8).reshape(1, -1), 0x06)[0].tobytes() == hashlib.sha3_256(m).digest()
    assert keccak256(np.zeros((1, 0), dtype=np.uint8))[0].tobytes().hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert keccak256(np.frombuffer(b"abc", dtype=np.uint8).reshape(1, -1))[0].tobytes().hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    # vectorised == one at a time
    msgs = np.frombuffer(bytes(range(200)) * 3, dtype=np.uint8).reshape(3, 200)
    assert all(keccak256(msgs)[i].tobytes() == keccak256(msgs[i:i + 1])[0].tobytes() for i in range(3))


# ---------------------------------------------------------------------------------- the model: KeccakHash<25>, Merkle, permutation
def digest25(h32):
    """[n][32] uint8 -> BytesHash<25> in four-word slots [n][4]: the first 25 bytes, zero padded."""
    w = np.ascontiguousarray(h32).view("<u8").astype(U64).reshape(-1, 4).copy()
    w[:, 3] &= U64(0xFF)
    return w


def model_hash_no_pad(rows):
    rows = np.asarray(rows, dtype=U64).reshape(len(rows), -1) % U64(P)
    return digest25(keccak256(np.ascontiguousarray(rows.astype("<u8")).view(np.uint8).reshape(rows.shape[0], -1)))


def model_hash_or_noop(rows):
    """plonk/config.rs:55-66 with HASH_SIZE = 25."""
    rows = np.asarray(rows, dtype=U64).reshape(len(rows), -1) % U64(P)
    if rows.shape[1] * 8 <= 25:
        out = np.zeros((rows.shape[0], 4), dtype=U64)
        out[:, :rows.shape[1]] = rows
        return out
    return model_hash_no_pad(rows)


def model_two_to_one(left, right):
    """hash/keccak.rs:119-126: Keccak-256 of the 50 bytes left || right."""
    lb = np.ascontiguousarray(np.asarray(left, dtype=U64).reshape(-1, 4)).view(np.uint8)[:, :25]
    rb = np.ascontiguousarray(np.asarray(right, dtype=U64).reshape(-1, 4)).view(np.uint8)[:, :25]
    return digest25(keccak256(np.concatenate([lb, rb], axis=1)))


def model_hash_elements(digests):
    """BytesHash::to_vec (hash_types.rs:181-191): chunks of 7, 7, 7, 4 bytes as little-endian integers."""
    out = []
    for d in np.asarray(digests, dtype=U64).reshape(-1, 4):
        b = d.astype("<u8").tobytes()[:25]
        out.append([int.from_bytes(b[i:i + 7], "little") for i in range(0, 25, 7)])
    return out


def model_hash_pad(elements):
    """plonk/config.rs:41-51."""
    v = list(elements) + [1]
    while (len(v) + 1) % 12:
        v.append(0)
    return model_hash_no_pad([v + [1]])[0]


def model_circuit_digest(cap, degree_bits):
    """circuit_builder.rs:1086-1098: hash_no_pad(cap.flatten() || hash_pad([]).to_vec() || [degree_bits])."""
    parts = [e for h in model_hash_elements(cap) for e in h] + model_hash_elements(model_hash_pad([]))[0] + [degree_bits]
    return model_hash_no_pad([parts])[0]


class ModelTree:
    """merkle_tree.rs:69-165: levels[0] = hash_or_noop of the leaves, levels[l + 1] = two_to_one of pairs."""

    def __init__(self, leaves):
        self.levels = [model_hash_or_noop(leaves)]
        while self.levels[-1].shape[0] > 1:
            d = self.levels[-1]
            self.levels.append(model_two_to_one(d[0::2], d[1::2]))

    def cap(self, cap_height):
        return self.levels[len(self.levels) - 1 - cap_height]

    def prove(self, index, cap_height):
        return np.array([self.levels[l][(index >> l) ^ 1] for l in range(len(self.levels) - 1 - cap_height)], dtype=U64).reshape(-1, 4)


def model_verify_path(leaf, index, siblings, cap):
    """merkle_proofs.rs:54-75."""
    cur = model_hash_or_noop([leaf])[0]
    for s in np.asarray(siblings, dtype=U64).reshape(-1, 4):
        cur = model_two_to_one(s, cur)[0] if index & 1 else model_two_to_one(cur, s)[0]
        index >>= 1
    return (cur == np.asarray(cap, dtype=U64).reshape(-1, 4)[index]).all()


def filter_words(words, want):
    """The rejection sampling of KeccakPermutation::permute (keccak.rs:84-94): words >= p are dropped; (elements, hashes consumed)."""
    out = []
    for i, w in enumerate(words):
        if len(out) == want:
            return out, (i + 3) // 4
        if w < P:
            out.append(w)
    assert len(out) == want
    return out, (len(words) + 3) // 4


def model_permute(state):
    """keccak.rs:64-95: the field elements of H(s) || H(H(s)) || ..., the first 12 that are < p."""
    h = keccak256(np.array([int(x) % P for x in state], dtype="<u8").view(np.uint8).reshape(1, 96))
    words = []
    while len([w for w in words if w < P]) < 12:
        words += [int(x) for x in h.view("<u8")[0]]
        h = keccak256(h)
    return filter_words(words, 12)[0]


def model_challenger():
    """iop/challenger.rs:30-153 over KeccakPermutation; a BytesHash<25> is observed as its four chunks."""
    return DuplexChallenger(model_permute, model_hash_elements)


def model_pow_responses(state, pos, candidates):
    """Element 7 of the onion for every candidate written to state[pos]: normally word 3 of the second hash."""
    st = np.tile(np.array([int(x) % P for x in state], dtype=U64), (len(candidates), 1))
    st[:, pos] = candidates
    h1 = keccak256(np.ascontiguousarray(st.astype("<u8")).view(np.uint8).reshape(len(candidates), 96))
    h2 = keccak256(h1)
    words = np.concatenate([h1.view("<u8"), h2.view("<u8")], axis=1).astype(U64)
    resp = words[:, 7].copy()
    for i in np.nonzero((words >= U64(P)).any(axis=1))[0]:           # a rejected word: follow the stream one state at a time
        s = [int(x) for x in st[i]]
        resp[i] = model_permute(s)[7]
    return resp


# ------------------------------------------------------------------------------------------------- C2: host entries against the model
LENGTHS = list(range(0, 41)) + [135, 139]


def noncanonical_rows(seed, count, length):
    r = np.random.default_rng(seed).integers(0, 2**64, (count, length), dtype=U64)
    if r.size:
        r.reshape(-1)[:: 3] |= U64(0xFFFFFFFF00000000)               # many words >= p: outputs are over canonical words
    return r


def test_host_hash_or_noop_and_two_to_one_match_the_model():
    import plonky2_demo_amd as p
    for length in LENGTHS:
        rows = noncanonical_rows(length, 5, length)
        got = p.hash_or_noop_host(rows, hasher=KECCAK)
        assert got.shape == (5, 4) and (got == model_hash_or_noop(rows)).all(), length
        assert (got[:, 3] >> U64(8) == 0).all()
    # the Poseidon form of the same entry is the device-independent hash_or_noop the verifier has always used
    l, r = model_hash_no_pad(noncanonical_rows(1, 40, 9)), model_hash_no_pad(noncanonical_rows(2, 40, 9))
    assert (p.two_to_one_host(l, r, hasher=KECCAK) == model_two_to_one(l, r)).all()
    assert (p.two_to_one_host(l[0], r[0], hasher=KECCAK) == model_two_to_one(l[:1], r[:1])[0]).all()
    # digests with all-ones bytes: the byte shift of the right half loses nothing
    ones = np.array([[2**64 - 1] * 3 + [0xFF]], dtype=U64)
    assert (p.two_to_one_host(ones, ones, hasher=KECCAK) == model_two_to_one(ones, ones)).all()
    # a non-zero padding byte (the 26th) is refused; so is another hasher
    bad = l[:1].copy()
    bad[0, 3] |= U64(1 << 8)
    with pytest.raises(p.Plonky2Mi355xError) as e:
        p.two_to_one_host(bad, r[:1], hasher=KECCAK)
    assert e.value.code == 1
    from plonky2_demo_amd._lib import lib
    out = np.zeros(4, dtype=U64)
    assert lib.gl_hash_or_noop_host(2, l.ctypes.data_as(ctypes.c_void_p), 1, 4, out.ctypes.data_as(ctypes.c_void_p)) == 1
    with pytest.raises(ValueError):
        p.hash_or_noop_host(l, hasher="sha256")


def test_host_poseidon_forms_of_the_new_entries_match_the_oracle(orc):
    import plonky2_demo_amd as p
    for length in (0, 1, 4, 5, 8, 9, 20, 135):
        rows = noncanonical_rows(100 + length, 3, length)
        got = p.hash_or_noop_host(rows, hasher="poseidon")
        assert all((got[i] == orc.hash_or_noop(rows[i])).all() for i in range(3))
    l, r = rand_field(5, (4, 4)), rand_field(6, (4, 4))
    got = p.two_to_one_host(l, r)
    assert all((got[i] == orc.two_to_one(l[i], r[i])).all() for i in range(4))


def test_hash_byte_helpers_round_trip():
    import plonky2_demo_amd as p
    d = model_hash_no_pad(noncanonical_rows(3, 6, 20))
    s = p.hash_to_bytes(d, KECCAK)
    assert all(len(x) == 25 for x in s) and (p.hash_from_bytes(s, KECCAK) == d).all()
    assert [list(map(int, e)) for e in p.hash_to_elements(d, KECCAK)] == model_hash_elements(d)
    q = rand_field(4, (3, 4))
    assert [len(x) for x in p.hash_to_bytes(q, "poseidon")] == [32] * 3 and (p.hash_from_bytes(p.hash_to_bytes(q, "poseidon"), "poseidon") == q).all()
    assert (p.hash_to_elements(q, "poseidon") == q).all()
    with pytest.raises(ValueError):
        p.hash_from_bytes([b"x" * 32], KECCAK)


def test_keccak_challenger_matches_the_model():
    # a script that crosses the rate several times, mixes elements, a Poseidon hash (4 elements) and Keccak hashes (7/7/7/4 bytes), and
    # asks for more than 8 challenges in a row
    import plonky2_demo_amd as p
    ch, mo = p.Challenger(hasher=KECCAK), model_challenger()
    rng = np.random.default_rng(7)
    pi_hash = rand_field(9, 4)
    cap = model_hash_no_pad(noncanonical_rows(11, 16, 30))
    assert ch.get_n_challenges(3) == mo.get(3)                       # a squeeze of the all-zero state
    for step in range(40):
        xs = rng.integers(0, 2**64, int(rng.integers(0, 21)), dtype=U64)
        ch.observe_elements(xs); mo.observe(xs)
        if step % 5 == 1:
            ch.observe_hashes(pi_hash, hasher="poseidon"); mo.observe(pi_hash)
        if step % 7 == 2:
            ch.observe_hashes(cap); mo.observe_hashes(cap)
        k = int(rng.integers(0, 6)) if step % 4 else 19
        assert ch.get_n_challenges(k) == mo.get(k)
        st, buf = ch.state()
        assert [int(x) % P for x in st] == mo.state and [int(x) % P for x in buf] == mo.inp
    bad = cap[:1].copy()
    bad[0, 3] |= U64(1 << 63)
    with pytest.raises(p.Plonky2Mi355xError):
        ch.observe_hashes(bad)
    from plonky2_demo_amd._lib import lib
    assert not lib.gl_challenger_new_h(2)


def test_desc_carries_the_hasher_and_verifier_only_bytes_round_trip():
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    from plonky2_demo_amd._lib import CircuitDesc, lib
    hk, hp = p.MatmulCircuit(2, hasher=KECCAK), p.MatmulCircuit(2)
    assert hk.desc.hasher == 1 and hp.desc.hasher == 0 and p.MatmulCircuit(2, zero_knowledge=True, hasher=KECCAK).desc.zero_knowledge == 1
    # the hasher is the LAST field: everything before it is the same description
    assert bytes(hk.desc)[:-8] == bytes(hp.desc)[:-8] and CircuitDesc.hasher.offset == CircuitDesc.num_gate_rows.offset + 4
    assert (hk.constants_sigmas() == hp.constants_sigmas()).all()
    h = ctypes.c_void_p()
    assert lib.gl_matmul_circuit_build_h(2, 0, 2, ctypes.byref(h)) == 1                     # hasher = 2 is refused
    # CommonCircuitData bytes do not hold the hasher: equal for both, and reading them gives 0
    assert api.common_data_to_bytes(hk.desc) == api.common_data_to_bytes(hp.desc)
    assert api.common_data_from_bytes(api.common_data_to_bytes(hk.desc))[0].hasher == 0
    # VerifierOnlyCircuitData: 25-byte hashes under Keccak; the Poseidon form of the new call is the old call byte for byte
    cap, dig = model_hash_no_pad(noncanonical_rows(21, 16, 30)), model_hash_no_pad(noncanonical_rows(22, 1, 30))[0]
    by = api.verifier_only_to_bytes(cap, dig, hasher=KECCAK)
    assert len(by) == 8 + 17 * 25 and by[8:] == b"".join(p.hash_to_bytes(np.vstack([cap, dig[None]]), KECCAK))
    cap2, dig2, used = api.verifier_only_from_bytes(by, hasher=KECCAK)
    assert (cap2 == cap).all() and (dig2 == dig).all() and used == len(by)
    pc, pd = rand_field(1, (16, 4)), rand_field(2, 4)
    old = np.empty(8 + 17 * 32, dtype=np.uint8)
    n = ctypes.c_size_t()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.gl_verifier_only_to_bytes(4, vp(pc), vp(pd), vp(old), old.size, ctypes.byref(n)) == 0
    assert api.verifier_only_to_bytes(pc, pd, hasher="poseidon") == old[: n.value].tobytes() == api.verifier_only_to_bytes(pc, pd)
    bad = cap.copy()
    bad[3, 3] |= U64(1 << 8)
    with pytest.raises(p.Plonky2Mi355xError):
        api.verifier_only_to_bytes(bad, dig, hasher=KECCAK)
    with pytest.raises(p.Plonky2Mi355xError):
        api.verifier_only_from_bytes(by[:-1], hasher=KECCAK)


# --------------------------------------------------------------------------------------------------------- C3: the rejection branch
def test_words_to_elements_rejection_branch_on_synthetic_streams(tmp_path):
    """kck_words_to_elements is shared by the host Challenger and the proof-of-work kernel.  A word >= p has probability 2^-32, so no
    real hash reaches its rejection branch: THIS test, over synthetic streams, is the only place it is exercised."""
    exe = str(tmp_path / "keccak_stream")
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else "c++"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "plonky2_demo_amd", "csrc"), os.path.join(ROOT, "tools", "keccak_stream.cpp"), "-o", exe])
    rng = np.random.default_rng(3)
    good = lambda k: [int(x) % P for x in rng.integers(0, 2**64, k, dtype=U64)]
    big = lambda k: [P + int(x) for x in rng.integers(0, 2**32 - 1, k, dtype=U64)]
    streams = {
        "none rejected": good(16),
        "position 0": big(1) + good(15),
        "position 7": good(7) + big(1) + good(12),
        "two in a row": good(2) + big(2) + good(12),
        "p itself and 2^64 - 1": good(3) + [P, 2**64 - 1] + good(15),
        "a fourth hash": big(1) + good(2) + big(1) + good(3) + big(1) + good(8),
        "a fifth hash": big(4) + good(3) + big(1) + good(12),
    }
    for name, words in streams.items():
        for want in (12, 8):
            r = subprocess.run([exe, str(want)] + ["%x" % w for w in words], capture_output=True, text=True)
            assert r.returncode == 0, (name, r.stderr)
            got = [int(x, 16) for x in r.stdout.split()]
            elems, used = filter_words(words, want)
            assert got[1:] == elems and got[0] == used, name
    assert filter_words(streams["a fourth hash"], 12)[1] == 4 and filter_words(streams["a fifth hash"], 12)[1] == 5
    assert subprocess.run([exe, "12"] + ["%x" % w for w in big(8)], capture_output=True).returncode == 1


# ------------------------------------------------------------------------------------------------- C4: kernels against the model
@pytest.mark.gpu
def test_gpu_hash_rows_match_the_model(gpu):
    p, ctx = gpu
    for length in LENGTHS:
        rows = noncanonical_rows(500 + length, 3000 if length in (17, 34, 135) else 300, length)
        got = p.hash_or_noop(rows, ctx=ctx, hasher=KECCAK)
        assert (got == model_hash_or_noop(rows)).all(), length
    with pytest.raises(ValueError):
        p.hash_or_noop(rows, ctx=ctx, hasher="blake")


@pytest.mark.gpu
def test_gpu_merkle_trees_match_the_model(gpu):
    p, ctx = gpu
    for leaf_len in (1, 3, 4, 17, 20, 135):
        for lg in range(13):
            n = 1 << lg
            leaves = noncanonical_rows(1000 * leaf_len + lg, n, leaf_len)
            mt = ModelTree(leaves)
            for cap_height in range(min(lg, 4) + 1):
                t = p.MerkleTree(leaves, cap_height, ctx=ctx, hasher=KECCAK)
                cap = t.cap
                assert (cap == mt.cap(cap_height)).all(), (leaf_len, lg, cap_height)
                for i in sorted({0, n - 1, n // 2, (n * 5) // 7, 1 % n}):
                    path = t.prove(i)
                    assert path.shape == (lg - cap_height, 4) and (path == mt.prove(i, cap_height)).all()
                if cap_height == min(lg, 4):
                    assert model_verify_path(leaves[n // 3], n // 3, t.prove(n // 3), cap)
                t.close()
    with pytest.raises(p.Plonky2Mi355xError):
        p.MerkleTree(leaves, 13, ctx=ctx, hasher=KECCAK)


@pytest.mark.gpu
def test_gpu_polynomial_batch_under_keccak(gpu, orc):
    from test_zero_knowledge import model_elements
    p, ctx = gpu
    for ncols, lg in ((20, 6), (135, 5), (2, 9)):
        vals = rand_field(40 + ncols, (ncols, 1 << lg))
        ob = orc.batch(vals, 3, 4, from_values=True, threads=4)
        gk = p.PolynomialBatch.from_values(vals, 3, False, 4, ctx=ctx, hasher=KECCAK)
        gp = p.PolynomialBatch.from_values(vals, 3, False, 4, ctx=ctx)
        assert gk.hasher == 1 and gp.hasher == 0
        assert (gk.polynomials == gp.polynomials).all() and (gk.polynomials == ob.polynomials).all()
        assert (gk.lde_values() == gp.lde_values()).all() and (gp.cap == ob.cap).all()
        leaves = ob.leaves()
        mt = ModelTree(leaves)
        assert (gk.cap == mt.cap(4)).all()
        for i in (0, 77, (8 << lg) - 1):
            assert (gk.get_leaf(i) == leaves[i]).all() and (gk.prove(i) == mt.prove(i, 4)).all()
        # from_coeffs, and the salted variant: leaves + the ChaCha model's salt columns (stream 0x200 + j, element = natural LDE row)
        gc = p.PolynomialBatch.from_coeffs(ob.polynomials, 3, False, 4, ctx=ctx, hasher=KECCAK)
        assert (gc.cap == gk.cap).all()
        seed = bytes(range(32))
        gs = p.PolynomialBatch.from_values_blinded(vals, 3, 4, seed=seed, ctx=ctx, hasher=KECCAK)
        N, lgN = 8 << lg, lg + 3
        rev = np.array([int(format(i, "0%db" % lgN)[::-1], 2) for i in range(N)])
        salt = np.stack([model_elements(seed, 0x200 + j, 0, N) for j in range(4)], axis=1)[rev]
        ms = ModelTree(np.concatenate([leaves, salt], axis=1))
        assert (gs.cap == ms.cap(4)).all() and (gs.get_leaf(5) == np.concatenate([leaves[5], salt[5]])).all()
        assert model_verify_path(gs.get_leaf(5), 5, gs.prove(5), gs.cap)


@pytest.mark.gpu
def test_gpu_pow_grind_finds_the_smallest_witness(gpu):
    p, ctx = gpu
    rng = np.random.default_rng(5)
    for k, (nbuf, bits) in enumerate(((1, 8), (7, 8), (3, 12), (5, 12), (0, 12), (2, 16), (6, 16))):
        state = rng.integers(0, 2**64, 12, dtype=U64)
        buf = rng.integers(0, 2**64, nbuf, dtype=U64)
        w = p.pow_grind(state, buf, bits, ctx=ctx, hasher=KECCAK)
        st = [int(x) for x in state]
        st[:nbuf] = [int(x) for x in buf]
        # exhaustive model search over every candidate up to the witness: it is valid AND minimal
        valid = []
        for base in range(0, w + 1, 1 << 16):
            cand = np.arange(base, min(base + (1 << 16), w + 1), dtype=U64)
            resp = model_pow_responses(st, nbuf, cand)
            valid += [int(c) for c, r in zip(cand, resp) if int(r) >> (64 - bits) == 0]
        assert valid == [w], (nbuf, bits, w, valid[:3])
        # the Challenger agrees: observing the witness yields a response with the leading zeros
        mo = model_challenger()
        mo.state, mo.inp = [x % P for x in [int(v) for v in state]], [int(x) % P for x in buf]
        mo.observe(np.array([w], dtype=U64))
        assert mo.get(1)[0] >> (64 - bits) == 0


# ------------------------------------------------------------------------------------------------------------ C5: whole proofs
def num_hashes(d):
    """The hashes a proof of description d holds: 3 + num_fri_rounds caps, the siblings of 4 initial and num_fri_rounds step paths per query."""
    lgN, cap = d.degree_bits + d.rate_bits, 1 << d.cap_height
    per_query, lg = 4 * (lgN - d.cap_height), lgN
    for r in range(d.num_fri_rounds):
        lg -= d.fri_arity_bits[r]
        per_query += lg - d.cap_height
    return (3 + d.num_fri_rounds) * cap + d.num_query_rounds * per_query


def poseidon_proof_len(d, npis):
    openings, leaf_words = sum(k for _, k in opening_columns(d)), sum(leaf_lens(d))
    final_len = (1 << d.degree_bits) >> sum(d.fri_arity_bits[r] for r in range(d.num_fri_rounds))
    per_query = 8 * leaf_words + 4 + sum(8 * (2 << d.fri_arity_bits[r]) + 1 for r in range(d.num_fri_rounds))
    return 32 * num_hashes(d) + 16 * openings + d.num_query_rounds * per_query + 16 * final_len + 8 + 8 + 8 * npis


def check_query_paths(d, pp, cs_cap, x_index, rounds):
    caps = [cs_cap] + pp.caps
    for q in rounds:
        init, steps = pp.queries[q]
        x = x_index[q]
        for o in range(4):
            assert model_verify_path(init[o][0], x, init[o][1], caps[o]), ("initial tree", q, o)
        for r, (leaf, sibs) in enumerate(steps):
            x >>= d.fri_arity_bits[r]
            assert model_verify_path(leaf, x, sibs, pp.fri_caps[r]), ("FRI tree", q, r)


def check_keccak_proof(p, orc, cd, d, proof, pis, wires=None, expect_caps=True):
    """C5 items 1-4 for one proof."""
    from plonky2_demo_amd import api
    by = proof.to_bytes()
    # 1. the three verifiers accept; the length is the Poseidon proof's minus 7 bytes per hash, from the description
    assert cd.verify(by) == (True, "")
    assert api.verify_bytes(api.verifier_data_to_bytes(d, cd.constants_sigmas_cap, cd.circuit_digest), by, hasher=KECCAK) == (True, "")
    assert len(by) == poseidon_proof_len(d, len(pis)) - 7 * num_hashes(d)
    # 4. circuit digest and constants/sigmas cap
    cs = cd.constants_sigmas_batch
    n, lgN = 1 << d.degree_bits, d.degree_bits + d.rate_bits
    if n <= 512:
        assert (cd.constants_sigmas_cap == ModelTree(orc.batch(cs.polynomials, 3, d.cap_height, from_values=False, threads=4).leaves()).cap(d.cap_height)).all()
    assert (cd.circuit_digest == model_circuit_digest(cd.constants_sigmas_cap, d.degree_bits)).all()
    # 2. independent transcript
    pp = ParsedProof(d, by)
    assert (pp.public_inputs == np.asarray(pis, dtype=U64)).all() and all((pp.caps[i] == proof.caps()[i]).all() for i in range(3))
    chal, response, x_index, _ = replay_transcript(d, model_challenger(), cd.circuit_digest, public_inputs_hash(orc, pis), pp)
    assert chal == proof.challenges()
    assert response >> (64 - d.proof_of_work_bits) == 0
    assert x_index == proof.query_indices()
    # 3. Merkle paths of the first and the last query round; caps over the oracle's LDE leaves for small circuits
    check_query_paths(d, pp, cd.constants_sigmas_cap, x_index, (0, d.num_query_rounds - 1))
    if expect_caps and n <= 512:
        cols = [proof.zs_partial_products(), None]
        if wires is not None:
            assert (pp.caps[0] == ModelTree(orc.batch(wires, 3, d.cap_height, from_values=True, threads=4).leaves()).cap(d.cap_height)).all()
        assert (pp.caps[1] == ModelTree(orc.batch(cols[0], 3, d.cap_height, from_values=True, threads=4).leaves()).cap(d.cap_height)).all()
        assert (pp.caps[2] == ModelTree(orc.batch(proof.quotient_chunks(), 3, d.cap_height, from_values=False, threads=4).leaves()).cap(d.cap_height)).all()
    return by, pp


def matmul_case(p, ctx, m, seed, zk=False, hasher=KECCAK):
    hc = p.MatmulCircuit(m, zero_knowledge=zk, hasher=hasher)
    a, b = rand_field(seed, m * m) % (2**32 - 1), rand_field(seed + 100, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=seed)
    return hc, hc.build(ctx), wires, pis


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 8, 64])
def test_keccak_matmul_proofs(gpu, orc, m):
    p, ctx = gpu
    hc, cd, wires, pis = matmul_case(p, ctx, m, 30 + m)
    assert cd.desc.hasher == 1
    proof = cd.prove(wires, pis)
    by, pp = check_keccak_proof(p, orc, cd, hc.desc, proof, pis, wires)
    assert hc.verify(by, cd.constants_sigmas_cap, cd.circuit_digest) == (True, "")
    # 5. the same witness under Poseidon is the oracle's proof; each proof is malformed under the other description
    hp, cdp, _, _ = matmul_case(p, ctx, m, 30 + m, hasher="poseidon")
    byp = cdp.prove(wires, pis).to_bytes()
    assert byp == orc.circuit(m, threads=8).witness(*[rand_field(30 + m + k, m * m) % (2**32 - 1) for k in (0, 100)], filler_seed=30 + m).prove(threads=8).to_bytes()
    assert len(byp) == poseidon_proof_len(hp.desc, len(pis)) == len(by) + 7 * num_hashes(hc.desc)
    for circuit, other in ((cd, byp), (cdp, by)):
        ok, why = circuit.verify(other)
        assert not ok and "malformed proof" in why
    ok, why = hp.verify(by, cd.constants_sigmas_cap, cd.circuit_digest)
    assert not ok and "malformed" in why


@pytest.mark.gpu
def test_keccak_zero_knowledge_proof(gpu, orc):
    p, ctx = gpu
    hc, cd, wires, pis = matmul_case(p, ctx, 2, 77, zk=True)
    buf = ctx.alloc(wires.nbytes).upload(wires)
    cd.blind_witness(buf.ptr, seed=bytes(range(32)))
    proof = cd.prove_device(buf.ptr, pis, seed=bytes(range(1, 33)))
    by, pp = check_keccak_proof(p, orc, cd, hc.desc, proof, pis, None, expect_caps=False)
    assert all(len(init[1][0]) == 139 and len(init[2][0]) == 24 and len(init[3][0]) == 20 for init, _ in pp.queries)
    assert by == cd.prove_device(buf.ptr, pis, seed=bytes(range(1, 33))).to_bytes()


def oracle_case(orc, kind, param):
    from test_verifier import merkle_proof_circuit_inputs
    oc = orc.circuit_of_kind(kind, param, threads=8)
    if kind == 8:
        w = oc.witness(np.arange(3, 3 + param, dtype=U64), np.zeros(0, dtype=U64), filler_seed=9)
    elif kind == 15:
        w = oc.witness(np.array([200, 300], dtype=U64), np.zeros(0, dtype=U64), filler_seed=4)
    else:
        w = oc.witness(merkle_proof_circuit_inputs(orc, param, 21)[0], np.zeros(0, dtype=U64), filler_seed=21)
    return oc, w


@pytest.mark.gpu
@pytest.mark.parametrize("kind,param", [(8, 50), (15, 9), (14, 6)])
def test_keccak_proofs_of_oracle_built_circuits(gpu, orc, kind, param):
    # a lookup circuit, the all-gates circuit and the Merkle-proof circuit: constants and sigmas from the oracle's builder, desc.hasher = 1
    p, ctx = gpu
    oc, w = oracle_case(orc, kind, param)
    d = oc.product_desc()
    assert d.hasher == 0                                             # existing descriptions stay Poseidon
    d.hasher = 1
    cd = p.GenericCircuitData(d, oc.constants_sigmas(), ctx)
    wires, pis = w.wires(), w.public_inputs()
    proof = cd.prove(wires, pis)
    check_keccak_proof(p, orc, cd, cd.desc, proof, pis, wires)
    d.hasher = 2
    with pytest.raises(p.Plonky2Mi355xError):
        p.GenericCircuitData(d, oc.constants_sigmas(), ctx)


@pytest.mark.gpu
def test_keccak_proof_tampering_is_rejected_with_the_check_named(gpu, orc):
    p, ctx = gpu
    hc, cd, wires, pis = matmul_case(p, ctx, 8, 55)
    d = hc.desc
    by = cd.prove(wires, pis).to_bytes()
    assert cd.verify(by) == (True, "")
    ncap, lgN = 1 << d.cap_height, d.degree_bits + d.rate_bits
    o_open = 3 * ncap * 25
    o_fcaps = o_open + 16 * sum(k for _, k in opening_columns(d))
    o_query = o_fcaps + d.num_fri_rounds * ncap * 25
    o_leaf0 = o_query                                                # first initial leaf (constants || sigmas row)
    o_sib0 = o_leaf0 + 8 * leaf_lens(d)[0] + 1                       # its first sibling
    o_pow = len(by) - 8 * len(pis) - 16

    def verdict(pos, bit=0):
        bad = bytearray(by)
        bad[pos] ^= 1 << bit
        return cd.verify(bytes(bad))

    # (a cap enters the transcript: every later challenge moves, and the identity at the new zeta is the first check to fail)
    for pos, what in ((5, "vanishing polynomial identity fails"), (o_sib0 + 3, "initial Merkle proof fails"), (o_leaf0 + 2, "initial Merkle proof fails"),
                      (o_pow, "invalid proof of work witness"), (o_open + 40, "vanishing polynomial identity fails")):
        ok, why = verdict(pos)
        assert not ok and what in why, (pos, why)
    # a non-zero 26th byte: the verifier data's hashes arrive in four-word slots
    cap = cd.constants_sigmas_cap.copy()
    cap[2, 3] |= U64(1 << 8)
    ok, why = hc.verify(by, cap, cd.circuit_digest)
    assert not ok and "malformed" in why
    dig = cd.circuit_digest.copy()
    dig[3] |= U64(1 << 40)
    ok, why = hc.verify(by, cd.constants_sigmas_cap, dig)
    assert not ok and "malformed" in why
    rng = np.random.default_rng(8)
    for _ in range(60):
        pos = int(rng.integers(0, len(by)))
        assert not verdict(pos, int(rng.integers(0, 8)))[0], pos
    assert not cd.verify(by + b"\0")[0] and not cd.verify(by[:-1])[0]


@pytest.mark.gpu
def test_keccak_phase_api_with_an_external_transcript(gpu, orc):
    # the lookup circuit of test_phase_api_on_a_lookup_circuit_with_an_external_transcript under desc.hasher = 1, with the library's
    # challenger and the Keccak grind entry: the bytes assembled by the caller equal gl_prove's
    p, ctx = gpu
    oc, w = oracle_case(orc, 8, 50)
    d = oc.product_desc()
    d.hasher = 1
    cd = p.GenericCircuitData(d, oc.constants_sigmas(), ctx)
    wires, pis = w.wires(), w.public_inputs()
    r = drive_phase_api(p, ctx, orc, cd, LibraryChallenger(p, KECCAK), wires, pis)
    assert r.zs_b.hasher == 1
    poseidon_wires = p.PolynomialBatch.from_device(r.d_wires.ptr, NUM_WIRES, cd.n, d.rate_bits, d.cap_height, True, ctx=ctx)
    with pytest.raises(p.Plonky2Mi355xError):                         # mixing hashers is GL_ERR_ARG
        cd.quotient_polys(poseidon_wires, r.zs_b, r.pi_hash, r.betas, r.gammas, r.alphas, deltas=r.deltas)
    with pytest.raises(p.Plonky2Mi355xError):
        cd.fri([r.batches[0], poseidon_wires, r.zs_b, r.q_b], r.zeta, r.fri_alpha)
    assert r.bytes == cd.prove(wires, pis).to_bytes()
    assert cd.verify(r.bytes) == (True, "")


@pytest.mark.gpu
def test_keccak_prover_pool_equals_single_stream_proofs(gpu):
    # 4 lanes x 16 proofs == the proofs made one at a time on the default context, byte for byte
    p, ctx = gpu
    m = 8
    hc = p.MatmulCircuit(m, hasher=KECCAK)
    cd = hc.build(ctx)
    ops, seeds, want = [], [], []
    for k in range(64):
        a, b = rand_field(3000 + k, m * m) % (2**32 - 1), rand_field(3100 + k, m * m) % (2**32 - 1)
        ops.append((a, b)); seeds.append(70 + k)
        wires, pis = hc.witness(a, b, filler_seed=70 + k)
        want.append(cd.prove(wires, pis).to_bytes())
    pool = p.ProverPool(hc, lanes=4)
    try:
        got = pool.prove_matmul(ops, seeds)
        assert [g.to_bytes() for g in got] == want
        assert (pool.circuit_digest == cd.circuit_digest).all()
    finally:
        pool.close()


GOLDEN = os.path.join(ROOT, "tests", "golden", "keccak_proof_hashes.json")


def keccak_golden_entries(p, ctx):
    out = {}
    for m, seed in ((1, 11), (3, 12), (8, 13)):                      # the seeds of tests/golden/proof_hashes.json
        hc = p.MatmulCircuit(m, hasher=KECCAK)
        a, b = rand_field(seed, m * m) % (2**32 - 1), rand_field(seed + 100, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=seed)
        cd = hc.build(ctx)
        pr = cd.prove(wires, pis)
        by = pr.to_bytes()
        assert cd.verify(by) == (True, "")
        out["m%d_seed%d" % (m, seed)] = {"sha256": hashlib.sha256(by).hexdigest(), "bytes": len(by), "pow_witness": pr.challenges()["pow_witness"],
                                         "digest": [int(x) for x in cd.circuit_digest]}
    return out


@pytest.mark.gpu
def test_keccak_proofs_match_the_recorded_hashes(gpu):
    """A REGRESSION PIN of this code against itself (recorded from the first green GPU run), not evidence of correctness: the model
    replay, the model trees and the verifiers above are the evidence."""
    p, ctx = gpu
    want = json.load(open(GOLDEN))
    assert keccak_golden_entries(p, ctx) == {k: v for k, v in want.items() if not k.startswith("_")}


@pytest.mark.gpu
def test_matrix_mul_example_accepts_under_keccak():
    exe = os.path.join(ROOT, "examples", "matrix_mul")
    for args in (["8", "1", "--keccak"], ["8", "1", "--keccak", "--zk"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "accepted" in r.stderr and "KeccakGoldilocksConfig" in r.stderr
        assert r.stdout.strip() == "length of proof.public_inputs is 192"               # matrix_mul.rs:90
