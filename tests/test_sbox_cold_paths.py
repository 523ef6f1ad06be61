"""The cold block of the Goldilocks product (gl64_gfx950.cuh glx_mul<false> / glx_mul3<false>) in EVERY S-box of the permutation and in
the kernels whose S-boxes tests/test_product_rare_fixup.py does not reach.

An S-box is x^2 = x x, x^4 = x^2 x^2, x^3 = x x^2, x^7 = x^3 x^4.  With the integer model of the product (test_product_rare_fixup.py
mul_model) the S-box input 2^48 makes x x subtract EPS without a carry (the cold block), 2^24 makes x^2 x^2 do so and 2^14 makes
x^3 x^4 do so; the operands of the cold product are 2^48, or 2^42 and 2^56, which have a single u64 representative, so this holds
whatever representative the kernel carries.  No simple input makes x x^2 cold (the edge grid and the sums and differences of two powers
of two were searched: no hit); that product meets borrow-only operands directly in tools/ubench/glx_check.hip.

The first S-box layer is reached by choosing the input (s[i] = value - RC[0][i]).  A later round is reached through the INVERSE of the
permutation (gen_poseidon_constants.perm_naive_to_input: the MDS inverse over the field and the 7th root x^(7^-1 mod p - 1)):
craft(round, value) is the input whose state right after the constants of `round` holds `value` in word 0 and random other words.
Rounds crafted: 3 (a full round inside the loop), 4 / 5 / 6 (the three data paths into psd_sbox of psd_partial_group<false>, group 0),
13 and 24 (first path of group 3, last path of the last group), 25 (the lone partial round), 26 and 29 (the last full rounds).

What cannot be crafted: the sponge and tree kernels (hash_or_noop, the Merkle kernels) fix the four capacity words of the state, which
leaves the inverse no freedom for deeper rounds; their crafted cases are the first S-box layer, as in test_product_rare_fixup.py.

GPU cases here: gl_poseidon_permute_raw with both MDS layers and poseidon() on the crafted rounds; k_pow_grind with every first-layer
S-box input at 2^48 / 2^24 / 2^14; k_merkle_leaves<WPE> and k_merkle_leaves_coop on hashed leaves with crafted first blocks.  (The
PoseidonGate kernel k_quotient<true>: tests/test_quotient_model.py.)  Every comparison is exact, against the CPU oracle."""
import os
import sys

import numpy as np
import pytest

from test_product_rare_fixup import P, SLOW, _crafted_states, _require_every_wave_takes_the_cold_block, mul_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_constants as g  # noqa: E402

# S-box input -> which of its four products (x x, x^2 x^2, x x^2, x^3 x^4) takes the cold block
COLD_VALUES = {1 << 48: 0, 1 << 24: 1, 1 << 14: 3}
CRAFTED_ROUNDS = [3, 4, 5, 6, 13, 24, 25, 26, 29]
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        rc = g.load_round_constants()
        M = g.mds_matrix()
        _TABLES = (rc, M, g.mat_inv(M))
    return _TABLES


def sbox_kinds(x):
    """the tail kinds of the four products of one S-box, chained on the words the model returns (as psd_sbox / psd_sbox_all)"""
    x2, k2 = mul_model(x, x)
    x4, k4 = mul_model(x2, x2)
    x3, k3 = mul_model(x, x2)
    _, k7 = mul_model(x3, x4)
    return [k2, k4, k3, k7]


def cold_products(state):
    """{(round, word, product)} of one permutation: the S-box products that take the cold block, from the Python trace"""
    rc, M, _ = tables()
    trace, _ = g.sbox_inputs([int(x) for x in state], rc, M)
    hits = set()
    for r, s in enumerate(trace):
        full = r < g.HALF_FULL or r >= g.HALF_FULL + g.N_PARTIAL
        for w in (range(12) if full else [0]):
            hits |= {(r, w, k) for k, kind in enumerate(sbox_kinds(s[w])) if kind == SLOW}
    return hits


def craft(round_, value, rng):
    """the 12-word input whose state right after the constants of `round_` has `value` in word 0 and random other words"""
    rc, _, Minv = tables()
    target = [value] + [int(x) for x in rng.integers(0, P, 11, dtype=np.uint64)]
    return g.perm_naive_to_input(target, round_, rc, Minv)


def crafted_permutation_inputs(count, seed):
    """`count` states, 64 to a wave.  In every wave lanes 0..26 are crafted -- one per (round, value) of CRAFTED_ROUNDS x COLD_VALUES, as
    far as the wave reaches --, lanes 30 and 31 are zero and the others random.  Returns (states, {index: (round, value)})."""
    rng = np.random.default_rng(seed)
    st = rng.integers(0, P, (count, 12), dtype=np.uint64)
    plan = [(r, v) for r in CRAFTED_ROUNDS for v in COLD_VALUES]
    where = {}
    for w0 in range(0, count, 64):
        for lane, (r, v) in enumerate(plan):
            if w0 + lane < count:
                # (rotated per wave, so that a one-lane last wave does not always repeat the first entry)
                r, v = plan[(lane + w0 // 64 * 5) % len(plan)]
                st[w0 + lane] = craft(r, v, rng)
                where[w0 + lane] = (r, v)
        for lane in (30, 31):
            if w0 + lane < count:
                st[w0 + lane] = 0
    return st, where


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_the_three_values_make_one_product_each_borrow_only():
    for value, product in COLD_VALUES.items():
        kinds = sbox_kinds(value)
        assert kinds[product] == SLOW and kinds.count(SLOW) == 1, (hex(value), kinds)
        if value + P < 1 << 64:                                                # the other u64 representative, where there is one
            assert sbox_kinds(value + P)[product] == SLOW
    # the cold product's operands have one u64 representative each
    assert mul_model(1 << 48, 1 << 48)[1] == SLOW and mul_model(1 << 42, 1 << 56)[1] == SLOW
    assert min(1 << 48, 1 << 42, 1 << 56) + P >= 1 << 64


def test_inverse_permutation_undoes_the_forward_one():
    rc, M, _ = tables()
    rng = np.random.default_rng(31)
    states = [[0] * 12, [P - 1] * 12, list(range(12))] + [[int(x) for x in rng.integers(0, P, 12, dtype=np.uint64)] for _ in range(5)]
    for s in states:
        out = g.perm_naive(s, rc, M)
        assert g.perm_naive_inverse(out, rc, M) == s
        assert g.perm_naive(g.perm_naive_inverse(s, rc, M), rc, M) == s
        trace, traced_out = g.sbox_inputs(s, rc, M)
        assert traced_out == out and len(trace) == 30 and trace[0] == [(a + c) % P for a, c in zip(s, rc[0])]


def test_forward_permutation_is_the_known_answers_and_the_oracle(golden, orc):
    rc, M, _ = tables()
    assert len(golden["poseidon_kats"]) == 4
    for kat in golden["poseidon_kats"]:
        assert g.perm_naive(kat["input"], rc, M) == kat["output"]
        assert g.perm_naive_inverse(kat["output"], rc, M) == [x % P for x in kat["input"]]
    st = np.random.default_rng(32).integers(0, P, (16, 12), dtype=np.uint64)
    want = orc.poseidon(st)
    for s, w in zip(st, want):
        assert g.perm_naive([int(x) for x in s], rc, M) == [int(x) for x in w]


def test_crafted_inputs_show_their_value_at_their_round():
    rc, M, _ = tables()
    rng = np.random.default_rng(33)
    for r in CRAFTED_ROUNDS + [0, 15]:
        for value, product in COLD_VALUES.items():
            s = craft(r, value, rng)
            assert all(0 <= x < P for x in s)
            trace, _ = g.sbox_inputs(s, rc, M)
            assert trace[r][0] == value
            assert (r, 0, product) in cold_products(s)


def _require_a_crafted_lane_in_every_wave(states, where):
    """from the Python trace: every crafted state takes the cold block at its round, in the product its value asks for, and every wave
    of 64 states holds at least one such lane next to lanes that never take it"""
    cold = {i: cold_products(states[i]) for i in range(len(states))}
    for i, (r, v) in where.items():
        assert (r, 0, COLD_VALUES[v]) in cold[i], "state %d does not reach the cold block in round %d" % (i, r)
    for w0 in range(0, len(states), 64):
        lanes = range(w0, min(w0 + 64, len(states)))
        assert any(i in where for i in lanes), "wave at %d has no crafted lane" % w0
        assert len(lanes) < 40 or any(not cold[i] for i in lanes)
    return cold


@pytest.mark.parametrize("count", [64, 65])
def test_crafted_waves_cover_every_round_and_value(count):
    st, where = crafted_permutation_inputs(count, 500 + count)
    cold = _require_a_crafted_lane_in_every_wave(st, where)
    assert {where[i] for i in where if i < 64} == {(r, v) for r in CRAFTED_ROUNDS for v in COLD_VALUES}
    assert not cold[30] and not cold[31] and (st[30] == 0).all()
    if count == 65:
        assert 64 in where


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("count", [64, 65])
def test_permutation_takes_the_cold_block_in_every_kind_of_round(gpu, orc, count):
    from test_poseidon_variants import LAYER_MFMA, LAYER_VALU, _permute_raw
    p, ctx = gpu
    st, where = crafted_permutation_inputs(count, 500 + count)
    _require_a_crafted_lane_in_every_wave(st, where)
    want = orc.poseidon(st)
    valu = _permute_raw(ctx, st, LAYER_VALU)
    mfma = _permute_raw(ctx, st, LAYER_MFMA)
    bad = np.argwhere((valu % np.uint64(P) != want).any(axis=1)).ravel()
    assert not len(bad), "VALU layer differs from the oracle at states %s (round, value): %s" % (bad[:6], [where.get(int(i)) for i in bad[:6]])
    assert (valu == mfma).all(), "the two layers leave different raw words at states %s" % np.argwhere((valu != mfma).any(axis=1)).ravel()[:6]
    assert (p.poseidon(st, ctx=ctx) == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("value", sorted(COLD_VALUES))
@pytest.mark.parametrize("bits", [6, 7, 8])
@pytest.mark.parametrize("buffer_len", [0, 5])
def test_pow_grind_with_every_first_layer_sbox_in_the_cold_block(gpu, orc, value, buffer_len, bits):
    # k_pow_grind: the caller gives the state.  Every word but the witness's enters its first S-box as `value`, in every lane of every wave.
    # (Every work level for each state: a wrong permutation can still agree on ONE smallest witness -- with the first layer's cold
    # products left unfixed, 2^14 / no pending input / 8 bits gives 291 either way -- but not on the smallest of all three levels.)
    p, ctx = gpu
    rc = tables()[0]
    state = np.array([(value - rc[0][i]) % P for i in range(12)], dtype=np.uint64)
    assert all((int(state[i]) + rc[0][i]) % P == value for i in range(12)) and sbox_kinds(value).count(SLOW) == 1
    witness = p.pow_grind(state, state[:buffer_len], bits, ctx=ctx)
    # the smallest w whose response has the leading zeros, scanned with the oracle
    want = None
    for base in range(0, 1 << 16, 1 << 12):
        cand = np.arange(base, base + (1 << 12), dtype=np.uint64)
        states = np.tile(state, (len(cand), 1))
        states[:, buffer_len] = cand
        ok = np.flatnonzero(orc.poseidon(states)[:, 7] >> np.uint64(64 - bits) == 0)
        if len(ok):
            want = int(cand[ok[0]])
            break
    assert want is not None and witness == want


def _bitrev(n):
    lg = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % lg)[::-1], 2) if lg else 0 for i in range(n)])


# 2^6 leaves: k_merkle_leaves_coop (16 lanes per leaf, four leaves to a wave); 2^14: k_merkle_leaves<WPE> (one leaf per lane), above the
# cooperative threshold of 8192.  Widths 8 (one full block), 9 (a second block of one word), 135 (17 blocks, the wires' width): all hashed
# (a leaf of at most 4 words is copied, not hashed).  Lane r of the launch hashes NATURAL row r = leaf bitrev(r).
@pytest.mark.gpu
@pytest.mark.parametrize("width", [8, 9, 135])
@pytest.mark.parametrize("lg,rows_per_wave", [(6, 4), (14, 64)])
def test_merkle_leaf_hashing_over_crafted_first_blocks(gpu, orc, lg, rows_per_wave, width):
    p, ctx = gpu
    n = 1 << lg
    rng = np.random.default_rng(600 + 10 * lg + width)
    natural = rng.integers(0, P, (n, width), dtype=np.uint64)
    first = np.zeros((n, 12), dtype=np.uint64)                       # the state of each row's first permutation: 8 words of the row, 4 zeros
    first[:, :8] = natural[:, :8]
    crafted_waves = sorted({0, (n // 64) // 3, n // 64 - 1})         # of 64 rows each
    for k, w in enumerate(crafted_waves):
        first[64 * w:64 * w + 64] = _crafted_states(64, 700 + lg + k, width=8)          # lanes 3, 17, 40 crafted, 5 and 6 zero
    natural[:, :8] = first[:, :8]
    for w in crafted_waves:
        for lane in (3, 17, 40):                                     # the wave (or cooperative wave of four rows) around each crafted row
            r0 = (64 * w + lane) // rows_per_wave * rows_per_wave
            _require_every_wave_takes_the_cold_block(first[r0:r0 + rows_per_wave], rows_per_wave, mixed=rows_per_wave == 64)
    rev = _bitrev(n)
    leaves = np.ascontiguousarray(natural[rev])                      # Merkle order: leaf j = natural row bitrev(j)
    gt = p.MerkleTree(leaves, 1, ctx=ctx)
    ot = orc.merkle(leaves, 1)
    assert (gt.cap == ot.cap).all()
    for w in crafted_waves:
        for lane in (3, 5, 17, 40):
            j = int(rev[64 * w + lane])
            assert (gt.prove(j) == ot.prove(j)).all()
    # and the digests of the crafted leaves themselves, one by one
    for w in crafted_waves:
        for lane in (3, 17, 40):
            row = natural[64 * w + lane]
            assert (p.hash_or_noop(row, ctx=ctx) == orc.hash_or_noop(row)).all()
