"""The Goldilocks product's rare borrow fix-up (gl64_gfx950.cuh glx_mul3 / glx_mul): the cold block inside the real kernels.

A product ends with y = lo + w2 EPS - hh, carry c, borrow b.  b without c ("subtract EPS") needs lo + w2 EPS < hh < 2^32: random
data reaches it about once in 2^32 products, so the kernels test the borrow masks of the wave (scalar, wave-uniform) and run the
two-sided tail only when one is set; otherwise the tail is r = y + EPS (c & ~b) (the non-canonical products, i.e. the S-boxes;
the canonical products of the NTT run the two-sided tail always).  The tests below drive crafted inputs through
that cold block: a state word s[i] = 2^48 - POSEIDON_RC[i] makes the first S-box square 2^48 (lo = 0, w2 = 0, hh = 1: borrow, no carry).

CPU: an integer model of the product as the kernels compute it (the same partial products, words, carry and borrow), the parent
commit's tail against the new one on the edge grid of tools/ubench/gl_prims.hip and on random pairs: identical u64 words.
GPU: poseidon(), hash_or_noop, Merkle trees (one lane per hash and the two cooperative kernels), field_op multiply and a 2^10
NTT against the CPU oracle / Python integers.  Every GPU case first counts with the model how many products of its batch take the
cold block -- the products of the first S-box layer, which the model reproduces word for word; later layers can only add -- and
requires at least one in every crafted wave, next to products that add EPS and products that need no fix-up."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = 0xFFFFFFFF00000001
EPS = 0xFFFFFFFF
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
SLOW, ADD, NONE = 0, 1, 2            # what a product's tail does: subtract EPS (the cold block) | add EPS | nothing


# ------------------------------------------------------------------------------------------------------- integer model
def product_parts(a, b):
    """(y, c, bw) of glx_mul3 / glx_mul for u64 a, b: y = lo + w2 EPS - hh (mod 2^64), the carry of the sum, the borrow of the difference."""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    p00, p11 = a0 * b0, a1 * b1
    mid = a0 * b1 + a1 * b0
    cm, mid = mid >> 64, mid & M64                       # the carry of the cross-term sum is worth 2^96 = -1
    s = (p00 >> 32) + (mid & M32); w1 = s & M32
    s = (p11 & M32) + (mid >> 32) + (s >> 32); w2 = s & M32
    w3 = (p11 >> 32) + (s >> 32)
    assert w3 <= M32
    z = (w1 << 32 | p00 & M32) + w2 * EPS
    c, z = z >> 64, z & M64
    hh = w3 + cm
    return (z - hh) & M64, c, 1 if z < hh else 0


def masks(y, c, bw, canon):
    n, p = bw & (1 - c), c & (1 - bw)
    if canon and not n and y > P - 1:
        p = 1
    return n, p


def tail_parent(y, c, bw, canon):
    """The two-sided tail (the parent commit's only tail, now the cold block): (f1:f0) = -EPS under n, +EPS under p, one 64-bit add."""
    n, p = masks(y, c, bw, canon)
    f1 = M32 if n else 0
    f0 = ((M32 if p else 0) - f1) & M32
    return (y + (f1 << 32 | f0)) & M64


def tail_fast(y, c, bw, canon):
    """The tail of a wave without a borrow-only lane: y + EPS p, NOT reduced mod 2^64 (the caller checks the range)."""
    n, p = masks(y, c, bw, canon)
    assert not n
    return y + EPS * p


def mul_model(a, b, canon=False):
    """(the u64 word the kernels return, SLOW / ADD / NONE)."""
    y, c, bw = product_parts(a, b)
    n, p = masks(y, c, bw, canon)
    return tail_parent(y, c, bw, canon), SLOW if n else ADD if p else NONE


def first_sbox_layer_kinds(state, rc0):
    """Tail kinds of the 48 products of the first S-box layer of one state (x^2, x^4, x^3, x^7 per word, as psd_sbox_all / psd_sbox)."""
    kinds = []
    for s, k in zip(state, rc0):
        x = int(s) + k
        if x > M64:                                      # gl_add_c
            x = (x & M64) + EPS
        x2, k2 = mul_model(x, x)
        x4, k4 = mul_model(x2, x2)
        x3, k3 = mul_model(x, x2)
        _, k7 = mul_model(x3, x4)
        kinds += [k2, k4, k3, k7]
    return kinds


def gl_prims_grid():
    """The edge grid of tools/ubench/gl_prims.hip main()."""
    g = [0, 1, 2, P - 1, P, P + 1, 0xFFFFFFFF, 0x100000000, M64, 0xFFFFFFFF00000000, 0xFFFFFFFEFFFFFFFF,
         0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE00000001, 0x00000001FFFFFFFF]
    for k in range(64):
        g += [1 << k, P - (1 << k)]
    for e in (36, 48, 60):
        g += [(h << (96 - e)) & M64 for h in (1, 3, 7, (1 << (e - 33)) + 1, (1 << (e - 32)) - 1)]
    g += [(0xFEDCBA9876543210 >> (64 - e)) << (64 - e) for e in (12, 24, 36, 48, 60)]
    return g


# ----------------------------------------------------------------------------------------------------------------- CPU
def _check_pairs(pairs):
    count = {SLOW: 0, ADD: 0, NONE: 0, "both": 0}
    for a, b in pairs:
        y, c, bw = product_parts(a, b)
        assert (y + (c - bw) * (1 << 64) - a * b) % P == 0            # the value the fix-up has to restore
        for canon in (False, True):
            want = tail_parent(y, c, bw, canon)
            assert want % P == a * b % P and (not canon or want < P)
            n, p = masks(y, c, bw, canon)
            if n:
                continue                                               # the kernels run the parent's tail itself
            got = tail_fast(y, c, bw, canon)
            assert got & M64 == want, "fast tail differs for %#x * %#x (canon %d)" % (a, b, canon)
            # y + EPS stays below 2^64 wherever a carry asks for it; only CANON's y >= p wraps, which is the subtraction of p it wants
            assert got <= M64 or (canon and not (c and not bw) and y >= P)
        n, p = masks(y, c, bw, False)
        count[SLOW if n else ADD if p else NONE] += 1
        count["both"] += c & bw
    return count


def test_fast_tail_equals_the_two_sided_tail_on_the_gl_prims_grid():
    g = gl_prims_grid()
    assert len(g) == 164
    count = _check_pairs((a, b) for a in g for b in g)
    # the grid is where the cold block is common: without these the comparison above would not have seen a borrow at all
    assert count[SLOW] > 400 and count["both"] > 400 and count[ADD] > 400, count


def test_fast_tail_equals_the_two_sided_tail_on_random_pairs():
    rng = np.random.default_rng(20)
    v = rng.integers(0, 2**64, (100_000, 2), dtype=np.uint64)
    count = _check_pairs((int(a), int(b)) for a, b in v)
    assert count[SLOW] == 0 and count[ADD] > 1000 and count[NONE] > 1000, count       # random data never takes the cold block


def test_square_of_2_to_the_48_borrows_without_a_carry():
    y, c, bw = product_parts(1 << 48, 1 << 48)
    assert (y, c, bw) == (M64, 0, 1)                                   # lo = 0, w2 = 0, hh = 1
    assert mul_model(1 << 48, 1 << 48) == ((1 << 96) % P, SLOW)


# ------------------------------------------------------------------------------------------------------ crafted inputs
def _rc0():
    import gen_poseidon_constants as g
    return g.load_round_constants()[0]


def _craft(state, words, rc0):
    for i in words:
        state[i] = (2**48 - rc0[i]) % P


def _crafted_states(count, seed, width=12):
    """`count` states, 64 to a wave: lane 3 crafted in word 0, lane 17 in words 2, 5, 7, lane 40 in every word, lanes 5 and 6 zero,
    the others random; the first lane of a last partial wave is crafted too."""
    rc0 = _rc0()
    rng = np.random.default_rng(seed)
    st = rng.integers(0, P, (count, 12), dtype=np.uint64)
    for w0 in range(0, count, 64):
        for lane, words in ((3, [0]), (17, [2, 5, 7]), (40, range(width)), (0, [1] if count - w0 < 4 else [])):
            if w0 + lane < count:
                _craft(st[w0 + lane], words, rc0)
        for lane in (5, 6):
            if w0 + lane < count:
                st[w0 + lane] = 0
    st[:, width:] = 0
    return st


def _require_every_wave_takes_the_cold_block(states, wave, mixed=True):
    """With the model: every wave of `wave` consecutive states has a product that takes the cold block -- and, in the same wave,
    products that add EPS and products without a fix-up (`mixed`)."""
    rc0 = _rc0()
    total = 0
    for w0 in range(0, len(states), wave):
        kinds = [k for s in states[w0:w0 + wave] for k in first_sbox_layer_kinds(s, rc0)]
        slow = kinds.count(SLOW)
        assert slow >= 1, "wave at %d never reaches the cold block" % w0
        if mixed:
            assert kinds.count(ADD) >= 1 and kinds.count(NONE) >= 1
        total += slow
    return total


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("count", [64, 65, 256])
def test_poseidon_on_crafted_states(gpu, orc, count):
    p, ctx = gpu
    st = _crafted_states(count, 100 + count)
    _require_every_wave_takes_the_cold_block(st, 64)
    got = p.poseidon(st, ctx=ctx)
    assert (got % np.uint64(P) == orc.poseidon(st)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("length", [8, 9, 135])
def test_hash_or_noop_on_rows_with_a_crafted_first_block(gpu, orc, length):
    p, ctx = gpu
    count = 70                                                          # k_hash_rows: a full wave and a partial one
    rng = np.random.default_rng(200 + length)
    rows = rng.integers(0, P, (count, length), dtype=np.uint64)
    first = _crafted_states(count, 300 + length, width=8)               # the state of the first permutation: 8 words of the row, 4 zeros
    rows[:, :8] = first[:, :8]
    _require_every_wave_takes_the_cold_block(first, 64)
    got = p.hash_or_noop(rows, ctx=ctx)
    want = np.stack([orc.hash_or_noop(r) for r in rows])
    assert (got == want).all()


# 2^6 leaves: the first level (32 nodes) is computed by k_merkle_top_coop; 2^8: by k_merkle_level_coop (128 nodes, above the top kernel's
# 64, below the cooperative threshold); 2^15: by k_merkle_level (16 384 nodes, above the threshold of 8192).  Each kernel's FIRST level is
# the one that reads the leaves, so each size puts the crafted pairs in front of another kernel; a digest above it is a hash output.
@pytest.mark.gpu
@pytest.mark.parametrize("lg,nodes_per_wave", [(6, 4), (8, 4), (15, 64)])
def test_merkle_build_over_crafted_digests(gpu, orc, lg, nodes_per_wave):
    p, ctx = gpu
    n = 1 << lg
    rng = np.random.default_rng(400 + lg)
    pairs = rng.integers(0, P, (n // 2, 12), dtype=np.uint64)          # two_to_one(l, r): the state is l, r, four zeros
    pairs[:, 8:] = 0
    rc0 = _rc0()
    crafted = sorted({1, 2, n // 4 + 1, n // 2 - 1})                    # nodes of the first level, in several waves / 16-lane groups
    for k, node in enumerate(crafted):
        _craft(pairs[node], [[0], [5], range(8), [3, 4]][k % 4], rc0)
    pairs[0] = 0
    for node in crafted:                                                # the wave (or the cooperative wave of four nodes) around it
        w0 = node // nodes_per_wave * nodes_per_wave
        _require_every_wave_takes_the_cold_block(pairs[w0:w0 + nodes_per_wave], nodes_per_wave)
    leaves = pairs[:, :8].reshape(n, 4)
    gt = p.MerkleTree(leaves, 0, ctx=ctx)
    ot = orc.merkle(leaves, 0)
    assert (gt.cap == ot.cap).all()
    for node in crafted:
        assert (gt.prove(2 * node) == ot.prove(2 * node)).all()
        assert (gt.prove((2 * node + 3) % n) == ot.prove((2 * node + 3) % n)).all()


@pytest.mark.gpu
def test_field_op_multiply_on_powers_of_two(gpu):
    p, ctx = gpu
    a, b = [], []
    for k in range(64):
        for j in range(64):
            a += [1 << k, P - (1 << k)]
            b += [1 << j, 1 << j]
    got = p.api.field_op(2, np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64), ctx=ctx)
    assert [int(x) for x in got] == [x * y % P for x, y in zip(a, b)]


@pytest.mark.gpu
def test_ntt_2_to_the_10_of_unit_vectors_and_powers_of_two(gpu, orc):
    # the butterflies' twiddle products are glx_mul3<true> / glx_mul<true>: the canonical tail, which keeps the two-sided fix-up
    p, ctx = gpu
    n = 1 << 10
    x = np.zeros((4, n), dtype=np.uint64)
    x[0, 1] = 1                                                          # a unit vector
    x[1, 5] = 1 << 48
    x[2] = np.array([1 << (i % 64) for i in range(n)], dtype=np.uint64)
    x[3] = np.array([P - (1 << (i % 64)) for i in range(n)], dtype=np.uint64)
    f = p.fft(x, ctx=ctx)
    assert (f == orc.fft(x)).all()
    assert (p.ifft(x, ctx=ctx) == orc.ifft(x)).all()
    assert (p.ifft(f, ctx=ctx) == x).all()
