"""Zero-knowledge proving: the keystream, blind_and_pad's layout, salted PolynomialBatches, salted proofs and their verification.

The randomness is pinned against a numpy ChaCha20 written from RFC 8439 (checked against the RFC's own vectors), the blinding layout
against a restatement of circuit_builder.rs:713-818, and every salted commitment against the CPU oracle's Merkle tree over leaves
built here.  The oracle cannot build a zero-knowledge circuit; whole zk proofs are pinned byte for byte against an integer derivation in
tests/test_zk_model.py, which shares the restatements of tests/zk_circuits.py with this file."""
import copy

import numpy as np
import pytest

from oracle_lib import P, rand_field
# the restatements shared with the zk model tests (tests/zk_circuits.py)
from zk_circuits import bitrev as _bitrev, blinding_counts, chacha20_blocks, fri_arity_bits, model_blinded_wires as _model_blinded_wires      # noqa: F401
from zk_circuits import model_elements, padded_degree_bits, salted_cap as _salted_cap      # noqa: F401

SEED = bytes(range(32))
SEED2 = bytes(range(100, 132))


def keystream_bytes(blocks):
    return blocks.astype("<u4").tobytes()


def test_chacha_model_matches_rfc8439_vectors():
    key = bytes(range(32))
    # 2.3.2: nonce 00:00:00:09:00:00:00:4a:00:00:00:00, block count 1
    blk = chacha20_blocks(key, (0x09000000, 0x4A000000, 0), [1])
    assert keystream_bytes(blk) == bytes.fromhex(
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    # 2.4.2: nonce 00:00:00:00:00:00:00:4a:00:00:00:00, initial counter 1: the first 64 bytes of the keystream (plaintext XOR ciphertext)
    pt = b"Ladies and Gentlemen of the class of '99: If I could offer you o"
    ct = bytes.fromhex("6e2e359a2568f98041ba0728dd0d6981e97e7aec1d4360c20a27afccfd9fae0b"
                       "f91b65c5524733ab8f593dabcd62b3571639d624e65152ab8f530c359f0861d8")
    ks = keystream_bytes(chacha20_blocks(key, (0, 0x4A000000, 0), [1]))
    assert bytes(a ^ b for a, b in zip(pt, ct)) == ks


def test_host_keystream_matches_rfc8439_appendix_vectors():
    import plonky2_demo_amd as p
    # A.1 test vectors 1 and 2: zero key, zero nonce (stream 0), block counters 0 and 1
    ks0 = bytes.fromhex("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
                        "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586")
    ks1 = bytes.fromhex("9f07e7be5551387a98ba977c732d080dcb0f29a048e3656912c6533e32ee7aed"
                        "29b721769ce64e43d57133b074d839d531ed1f28510afb45ace10a1f4b794d6f")
    for blk, ks in ((0, ks0), (1, ks1)):
        w = np.frombuffer(ks, dtype="<u8")
        want = [(int(w[2 * j]) + (int(w[2 * j + 1]) << 64)) % P for j in range(4)]
        assert [int(x) for x in p.random_elements(bytes(32), 0, 4 * blk, 4, ctx=False)] == want
    assert keystream_bytes(chacha20_blocks(bytes(32), (0, 0, 0), [0, 1])) == ks0 + ks1


@pytest.mark.parametrize("stream,first,count", [(0x100, 0, 64), (0x100 + 134, 3, 29), (0x200 + 4 + 3, 1021, 7), (0x20F, 5, 1),
                                                (7, (1 << 20) + 2, 10)])
def test_host_elements_match_the_model(stream, first, count):
    import plonky2_demo_amd as p
    got = p.random_elements(SEED, stream, first, count, ctx=False)
    assert (got == model_elements(SEED, stream, first, count)).all()
    assert (got < P).all()
    # any sub-range is the same slice of the stream
    assert (p.random_elements(SEED, stream, first + 1, count - 1, ctx=False) == got[1:]).all()


# ---------------------------------------------------------------------------------------------------- blinding layout
def first_occurrence_labels(classes):
    """A copy-class matrix relabelled by first occurrence: equal labels = the same partition, whatever ids the builder used."""
    flat = classes.reshape(-1)
    _, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(first.size)
    return rank[inv.reshape(-1)].reshape(classes.shape)


def wire_classes(hc):
    import ctypes
    from plonky2_demo_amd._lib import lib, check
    out = np.empty((80, hc.n), dtype=np.uint64)
    check(lib.gl_host_circuit_wire_classes(hc.handle, out.ctypes.data_as(ctypes.c_void_p)))
    return out


TABLE = {2: (6, 2774, 2776, 14, 3), 8: (75, 2774, 2776, 14, 7), 16: (495, 2774, 2776, 14, 9), 64: (27549, 3446, 3448, 16, 15),
         128: (215043, 3614, 3616, 18, 18)}


def test_blinding_counts_restatement_reproduces_the_table():
    for m, (rows, regular, pairs, lg_zk, lg_plain) in TABLE.items():
        assert blinding_counts(rows) == (regular, pairs)
        assert padded_degree_bits(rows, True) == lg_zk and padded_degree_bits(rows, False) == lg_plain


@pytest.mark.parametrize("m", [1, 2, 8, 64, 128])
def test_zk_matmul_layout(m):
    import plonky2_demo_amd as p
    plain, zk = p.MatmulCircuit(m), p.MatmulCircuit(m, zero_knowledge=True)
    d, dz = plain.desc, zk.desc
    g = dz.num_gate_rows
    assert d.zero_knowledge == 0 and d.num_gate_rows == 0 and dz.zero_knowledge == 1
    pg = plain.row_gates()
    assert g == int(np.nonzero(pg)[0][-1]) + 1                      # the constant row is the last gate row
    if m in TABLE:
        assert g == TABLE[m][0] and dz.degree_bits == TABLE[m][3] and d.degree_bits == TABLE[m][4]
    assert dz.degree_bits == padded_degree_bits(g, True) and d.degree_bits == padded_degree_bits(g, False)
    assert list(dz.fri_arity_bits)[:dz.num_fri_rounds] == fri_arity_bits(dz.degree_bits)
    assert not any(dz.fri_arity_bits[dz.num_fri_rounds:])
    # the rest of the description is the plain one
    for f in ("num_wires", "num_routed_wires", "num_constants", "num_selectors", "num_public_inputs", "rate_bits", "cap_height",
              "num_query_rounds", "proof_of_work_bits"):
        assert getattr(d, f) == getattr(dz, f), f
    # the gate set: the plain one, plus NoopGate (sorted first) when the plain rows fill a power of two without padding (m = 1)
    plain_gates, zk_gates = list(d.gate_types)[:d.num_gates], list(dz.gate_types)[:dz.num_gates]
    same_gate_set = plain_gates == zk_gates
    assert same_gate_set or (plain_gates[0] != 0 and zk_gates == [0] + plain_gates and g == plain.n)
    # rows below num_gate_rows: the plain build's gates, constants and copy classes; from there on NoopGate rows, singleton classes
    zg = zk.row_gates()
    assert (zg[:g] == pg[:g]).all() and (zg[g:] == 0).all()
    nc = d.num_constants
    cs, csz = plain.constants_sigmas(), zk.constants_sigmas()
    ns = d.num_selectors
    assert (csz[ns:nc, :g] == cs[ns:nc, :g]).all() and (csz[ns:nc, g:] == 0).all()      # gate constants
    if same_gate_set:
        assert (csz[:ns, :g] == cs[:ns, :g]).all()                  # selectors
        assert (csz[:nc, g:] == cs[:nc, -1:]).all()                 # a padding row's constants (Noop selectors)
    else:
        gate_at = lambda desc, col: np.array([desc.gate_types[v] if v < desc.num_gates else 255 for v in col.tolist()])
        for k in range(ns):
            assert (gate_at(dz, csz[k, :g]) == gate_at(d, cs[k, :g])).all()
    wc, wcz = wire_classes(plain), wire_classes(zk)
    assert (first_occurrence_labels(wcz[:, :g]) == first_occurrence_labels(wc[:, :g])).all()
    ids, counts = np.unique(wcz, return_counts=True)
    assert (counts[np.searchsorted(ids, wcz[:, g:].reshape(-1))] == 1).all()
    # sigma is the identity on the blinding rows: sigma(row, col) = k_col * w^row
    root = 1753635133440165772
    for _ in range(32 - dz.degree_bits):
        root = root * root % P
    for r in (g, g + 1, zk.n - 1):
        for c in (0, 79):
            assert int(csz[nc + c, r]) == dz.k_is[c] * pow(root, r, P) % P


# ---------------------------------------------------------------------------------------------------- wire format
def _flag_offsets(desc):
    fri = 3 * 8 + 4 + 1 + 16
    return 6 * 8 + 1, 6 * 8 + 2 + fri + fri + 8 + 8 * desc.num_fri_rounds + 8


def test_zk_common_data_round_trips_and_mixed_flags_are_refused():
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    hc = p.MatmulCircuit(2, zero_knowledge=True)
    by = api.common_data_to_bytes(hc.desc)
    zk_at, hiding_at = _flag_offsets(hc.desc)
    assert by[zk_at] == 1 and by[hiding_at] == 1
    plain = api.common_data_to_bytes(p.MatmulCircuit(2).desc)
    assert plain[zk_at] == 0 and plain[_flag_offsets(p.MatmulCircuit(2).desc)[1]] == 0
    d2, used = api.common_data_from_bytes(by)
    assert used == len(by) and d2.zero_knowledge == 1 and d2.num_gate_rows == 0
    want = copy.copy(hc.desc)
    want.num_gate_rows = 0                                            # not part of CommonCircuitData
    assert bytes(d2) == bytes(want)
    assert api.common_data_to_bytes(d2) == by
    for at in (zk_at, hiding_at):
        bad = bytearray(by)
        bad[at] = 0
        with pytest.raises(p.Plonky2Mi355xError) as e:
            api.common_data_from_bytes(bytes(bad))
        assert e.value.code == 3


# ---------------------------------------------------------------------------------------------------- GPU
def _zk_proof(p, ctx, hc, cd, a, b, seed, filler_seed=5):
    wires, pis = hc.witness(a, b, filler_seed=filler_seed)
    buf = ctx.alloc(135 * hc.n * 8)
    buf.upload(wires)
    cd.blind_witness(buf.ptr, seed=seed)
    blinded = buf.download((135, hc.n))
    proof = cd.prove_device(buf.ptr, pis, seed=seed)
    buf.free()
    return wires, pis, blinded, proof


def _wire_openings(proof_bytes, desc):
    off = 3 * 4 * (1 << desc.cap_height) + 2 * desc.num_constants + 2 * 80      # caps, constants, sigmas: whole words
    return np.frombuffer(proof_bytes, dtype="<u8", count=off + 2 * 135)[off:].copy()


@pytest.mark.gpu
def test_device_keystream_matches_the_model(gpu):
    p, ctx = gpu
    for stream, first, count in ((0x100, 0, 4096), (0x20B, 3, 1001), (0x100 + 77, (1 << 21) - 5, 300)):
        got = p.random_elements(SEED, stream, first, count, ctx=ctx)
        assert (got == model_elements(SEED, stream, first, count)).all()
        assert (got == p.random_elements(SEED, stream, first, count, ctx=False)).all()


@pytest.mark.gpu
def test_salted_polynomial_batch(gpu, orc):
    p, ctx = gpu
    vals = rand_field(31, (20, 1 << 9))
    B = p.PolynomialBatch
    for from_values in (True, False):
        make, blinded = (B.from_values, B.from_values_blinded) if from_values else (B.from_coeffs, B.from_coeffs_blinded)
        gb, plain = blinded(vals, 3, 4, ctx=ctx), make(vals, 3, False, 4, ctx=ctx)
        ob = orc.batch(vals, 3, 4, from_values=from_values, threads=8)
        assert (gb.polynomials == ob.polynomials).all() and (gb.lde_values() == plain.lde_values()).all()
        N = (1 << 9) << 3
        leaves = np.stack([gb.get_leaf(i) for i in range(N)])
        assert leaves.shape == (N, 24)
        assert (leaves[:, :20] == ob.leaves()).all()
        for i in (0, 5, 1234, N - 1):
            assert (gb.get_lde_values(i, 1) == plain.get_lde_values(i, 1)).all()
            assert (gb.get_lde_values(i, 1) == ob.leaves()[_bitrev(12)[i]]).all()
        tree = orc.merkle(leaves, 4)
        assert (gb.cap == tree.cap).all() and not (gb.cap == plain.cap).all()
        for i in (0, 77, N - 1):
            assert orc.merkle_verify(leaves[i], i, gb.cap, gb.prove(i))
        # a fresh OS seed per batch; with a seed, salt column j is stream 0x200 + j
        again = blinded(vals, 3, 4, ctx=ctx)
        assert not (again.cap == gb.cap).all()
        seeded = blinded(vals, 3, 4, seed=SEED, ctx=ctx)
        assert (seeded.cap == _salted_cap(orc, vals, from_values, 0, SEED)).all()
        # the reference entries keep refusing blinding
        with pytest.raises(p.Plonky2Mi355xError) as e:
            make(vals, 3, True, 4, ctx=ctx)
        assert e.value.code == 3


@pytest.mark.gpu
def test_zk_proof_commitments_are_pinned_and_verified(gpu, orc):
    p, ctx = gpu
    from plonky2_demo_amd import api
    m = 2
    hc = p.MatmulCircuit(m, zero_knowledge=True)
    cd = hc.build(ctx)
    a, b = rand_field(3, m * m) % (2**32 - 1), rand_field(4, m * m) % (2**32 - 1)
    wires, pis, blinded, proof = _zk_proof(p, ctx, hc, cd, a, b, SEED)
    g = hc.desc.num_gate_rows
    expected = _model_blinded_wires(wires, g, SEED)
    assert (blinded == expected).all()
    by = proof.to_bytes()
    assert cd.verify(proof) == (True, "")
    assert hc.verify(by, cd.constants_sigmas_cap, cd.circuit_digest) == (True, "")
    vd = api.verifier_data_to_bytes(hc.desc, cd.constants_sigmas_cap, cd.circuit_digest)
    assert api.verify_bytes(vd, by) == (True, "")
    caps = proof.caps()
    assert (caps[0] == _salted_cap(orc, expected, True, 1, SEED)).all()
    assert (caps[1] == _salted_cap(orc, proof.zs_partial_products(), True, 2, SEED)).all()
    assert (caps[2] == _salted_cap(orc, proof.quotient_chunks(), False, 3, SEED)).all()
    # tampering: one salt word of the first query's wires leaf
    d = hc.desc
    ncap, nsib = 1 << d.cap_height, d.degree_bits + d.rate_bits - d.cap_height
    words = 3 * 4 * ncap + 2 * (d.num_constants + 80 + 135 + 2 + 2 + 18 + 16) + d.num_fri_rounds * 4 * ncap
    at = 8 * words + 8 * (d.num_constants + 80) + 1 + 8 * 4 * nsib + 8 * 135
    bad = bytearray(by)
    bad[at] ^= 1
    ok, why = cd.verify(bytes(bad))
    assert not ok and why.startswith("initial Merkle proof fails")
    # the zk description with zero_knowledge cleared expects unsalted leaves of the same n: malformed
    unsalted = copy.copy(d)
    unsalted.zero_knowledge, unsalted.num_gate_rows = 0, 0
    import ctypes
    from plonky2_demo_amd._lib import lib
    buf = np.frombuffer(by, dtype=np.uint8)
    st = lib.gl_verify(ctypes.byref(unsalted), cd.constants_sigmas_cap.ctypes.data_as(ctypes.c_void_p),
                       cd.circuit_digest.ctypes.data_as(ctypes.c_void_p), buf.ctypes.data_as(ctypes.c_void_p), buf.size)
    assert st == 6 and lib.gl_last_error().decode().startswith("malformed proof")


@pytest.mark.gpu
def test_zk_proofs_are_deterministic_per_seed_and_hide_per_seed(gpu):
    p, ctx = gpu
    m = 2
    hc = p.MatmulCircuit(m, zero_knowledge=True)
    cd = hc.build(ctx)
    ctx2 = p.Context(0)
    cd2 = p.api.CircuitView(cd, ctx2)
    a, b = rand_field(13, m * m) % (2**32 - 1), rand_field(14, m * m) % (2**32 - 1)
    _, _, _, p1 = _zk_proof(p, ctx, hc, cd, a, b, SEED)
    _, _, _, p1b = _zk_proof(p, ctx2, hc, cd2, a, b, SEED)
    _, _, _, p2 = _zk_proof(p, ctx, hc, cd, a, b, SEED2)
    assert p1.to_bytes() == p1b.to_bytes()
    c1, c2 = p1.caps(), p2.caps()
    for k in range(3):
        assert not (c1[k] == c2[k]).any()
    o1, o2 = _wire_openings(p1.to_bytes(), hc.desc), _wire_openings(p2.to_bytes(), hc.desc)
    assert not (o1 == o2).all()
    for pr in (p1, p2):
        assert cd.verify(pr) == (True, "")
    # without a seed: OS entropy, a different proof every time
    _, _, _, p3 = _zk_proof(p, ctx, hc, cd, a, b, None)
    assert cd.verify(p3) == (True, "") and p3.to_bytes() != p1.to_bytes()


@pytest.mark.gpu
def test_zk_prover_pool(gpu):
    p, _ = gpu
    m = 2
    hc = p.MatmulCircuit(m, zero_knowledge=True)
    pool = p.ProverPool(hc, lanes=4)
    a, b = rand_field(21, m * m) % (2**32 - 1), rand_field(22, m * m) % (2**32 - 1)
    proofs = [pr.to_bytes() for pr in pool.prove_matmul([(a, b)] * 16, filler_seeds=[9] * 16)]
    assert len(set(proofs)) == 16
    for by in proofs:
        assert hc.verify(by, pool.constants_sigmas_cap, pool.circuit_digest) == (True, "")


@pytest.mark.gpu
def test_zk_phase_api_is_refused(gpu):
    p, ctx = gpu
    hc = p.MatmulCircuit(2, zero_knowledge=True)
    cd = hc.build(ctx)
    buf = ctx.alloc(135 * hc.n * 8)
    with pytest.raises(p.Plonky2Mi355xError) as e:
        cd.partial_products(buf.ptr, [1, 2], [3, 4])
    assert e.value.code == 3
    buf.free()


@pytest.mark.gpu
def test_zk_m64(gpu):
    p, ctx = gpu
    m = 64
    hc = p.MatmulCircuit(m, zero_knowledge=True)
    assert hc.n == 1 << 16
    cd = hc.build(ctx)
    a, b = rand_field(41, m * m) % (2**32 - 1), rand_field(42, m * m) % (2**32 - 1)
    buf = ctx.alloc(135 * hc.n * 8)
    gen = hc.witness_generator(ctx)
    pis = gen.run(a, b, buf.ptr, filler_seed=3)
    cd.blind_witness(buf.ptr)
    proof = cd.prove_device(buf.ptr, pis)
    buf.free()
    assert cd.verify(proof) == (True, "")


@pytest.mark.gpu
def test_generic_circuit_blinded_like_a_rust_zk_build(gpu, orc):
    # what a Rust-built zk circuit looks like: the plain gate rows, then blinding rows and padding (NoopGates, identity sigma)
    p, ctx = gpu
    from plonky2_demo_amd import api
    from test_verifier import merkle_proof_circuit_inputs
    height, index = 4, 11
    oc = orc.circuit_of_kind(14, height, threads=8)
    a, _root = merkle_proof_circuit_inputs(orc, height, index)
    w = oc.witness(a, np.zeros(0, dtype=np.uint64), filler_seed=height)
    desc, cs = oc.product_desc(), oc.constants_sigmas()
    n = oc.n
    rows = oc.row_gates()
    g = int(np.nonzero(rows)[0][-1]) + 1
    assert g < n and desc.gate_types[0] == 0                          # a NoopGate padding row exists to copy constants from
    lg = padded_degree_bits(g, True)
    n2 = 1 << lg
    zd = copy.copy(desc)
    zd.degree_bits, zd.zero_knowledge, zd.num_gate_rows = lg, 1, g
    ar = fri_arity_bits(lg)
    zd.num_fri_rounds = len(ar)
    for i in range(8):
        zd.fri_arity_bits[i] = ar[i] if i < len(ar) else 0
    nc = desc.num_constants
    root_n, root_n2 = orc.primitive_root(desc.degree_bits), orc.primitive_root(lg)
    assert pow(int(root_n2), n2 // n, P) == int(root_n)
    decode = {}
    for j in range(80):
        for r in range(n):
            decode[desc.k_is[j] * pow(int(root_n), r, P) % P] = (j, r)
    cs2 = np.zeros((nc + 80, n2), dtype=np.uint64)
    cs2[:nc, :g] = cs[:nc, :g]
    cs2[:nc, g:] = cs[:nc, n - 1:n]
    for c in range(80):
        for r in range(n2):
            j, rr = decode[int(cs[nc + c, r])] if r < g else (c, r)
            cs2[nc + c, r] = zd.k_is[j] * pow(int(root_n2), rr, P) % P
    cd = p.GenericCircuitData(zd, cs2, ctx=ctx)
    wires = np.zeros((135, n2), dtype=np.uint64)
    wires[:, :g] = w.wires()[:, :g]
    buf = ctx.alloc(135 * n2 * 8)
    buf.upload(wires)
    cd.blind_witness(buf.ptr, seed=SEED)
    assert (buf.download((135, n2)) == _model_blinded_wires(wires, g, SEED)).all()
    proof = cd.prove_device(buf.ptr, w.public_inputs(), seed=SEED)
    buf.free()
    assert cd.verify(proof) == (True, "")
    read, _ = api.common_data_from_bytes(api.common_data_to_bytes(zd))
    vd = api.verifier_data_to_bytes(read, cd.constants_sigmas_cap, cd.circuit_digest)
    assert api.verify_bytes(vd, proof.to_bytes()) == (True, "")
    # a description whose degree_bits does not follow from num_gate_rows is refused
    bad = copy.copy(zd)
    bad.num_gate_rows = g + 20000
    with pytest.raises(p.Plonky2Mi355xError):
        p.GenericCircuitData(bad, cs2, ctx=ctx)


@pytest.mark.gpu
def test_demo_binary_zk(gpu):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([os.path.join(root, "examples", "matrix_mul"), "8", "1", "--zk"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "zero knowledge" in r.stderr and "accepted" in r.stderr
