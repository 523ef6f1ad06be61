"""GPU parity tests (-m gpu): the HIP path through the C ABI against the CPU oracle, the committed golden
fixtures and size-independent properties.  Bit-exact: all values are canonical u64."""
import numpy as np
import pytest

from oracle_lib import P, rand_field
from transcript import LibraryChallenger, drive_phase_api, poseidon_challenger

pytestmark = pytest.mark.gpu


def ints(a):
    return [int(x) for x in np.asarray(a).reshape(-1)]


# ------------------------------------------------------------------------------------------------ field
def test_field_ops_edge_grid(gpu, orc, golden):
    p, ctx = gpu
    from plonky2_demo_amd import api
    g = golden["field_grid"]
    a = np.array([x for x in g for _ in g], dtype=np.uint64)
    b = np.array([y for _ in g for y in g], dtype=np.uint64)
    c = np.roll(a, 7)
    for op in (0, 1, 2):
        assert (api.field_op(op, a, b) == orc.field_op(op, a, b)).all(), op
    assert (api.field_op(6, a, b, c) == orc.field_op(6, a, b, c)).all()
    ga = np.array(g, dtype=np.uint64)
    assert (api.field_op(3, ga) == orc.field_op(3, ga)).all()
    assert (api.field_op(5, ga) == orc.field_op(5, ga)).all()
    nz = np.array([x for x in g if x % P], dtype=np.uint64)
    assert (api.field_op(4, nz) == orc.field_op(4, nz)).all()
    # x * 2^e for all 192 exponents on the grid (shift-twiddles of the NTT butterflies)
    e = np.arange(192, dtype=np.uint64)
    xs = np.repeat(ga, 192)
    es = np.tile(e, len(g))
    got = api.field_op(7, xs, es)
    assert ints(got) == [int(x) * pow(2, int(k), P) % P for x, k in zip(xs, es)]


def test_field_ops_random(gpu, orc):
    from plonky2_demo_amd import api
    a = np.random.default_rng(1).integers(0, 2**64, size=1 << 16, dtype=np.uint64)   # non-canonical inputs allowed
    b = np.random.default_rng(2).integers(0, 2**64, size=1 << 16, dtype=np.uint64)
    c = np.random.default_rng(3).integers(0, 2**64, size=1 << 16, dtype=np.uint64)
    for op in (0, 1, 2):
        assert (api.field_op(op, a, b) == orc.field_op(op, a, b)).all(), op
    assert (api.field_op(6, a, b, c) == orc.field_op(6, a, b, c)).all()
    ea, eb = rand_field(4, 4096), rand_field(5, 4096)
    for op in (0, 1, 2):
        assert (api.ext_op(op, ea, eb) == orc.ext_op(op, ea, eb)).all(), op
    assert (api.ext_op(3, ea) == orc.ext_op(3, ea)).all()


# -------------------------------------------------------------------------------------------------- NTT
def test_fft_reference_test_case(gpu, golden):
    p, ctx = gpu
    c = np.array(golden["fft256"]["coeffs"], dtype=np.uint64)
    v = p.fft(c)
    assert ints(v) == golden["fft256"]["values"]          # field/src/fft.rs:234-235
    assert (p.ifft(v) == c).all()                          # :237-243
    for case in golden["ntt_model"]:
        cc = np.array(case["coeffs"], dtype=np.uint64)
        assert ints(p.fft(cc)) == case["values"]
        assert ints(p.coset_fft(cc, 7)) == case["coset7"]
    m = golden["lde_model"]
    assert ints(p.lde_onto_coset(np.array(m["coeffs"], dtype=np.uint64), m["rate_bits"])) == m["values"]


@pytest.mark.parametrize("lg", list(range(0, 17)))
def test_ntt_matches_oracle_all_sizes(gpu, orc, lg):
    p, ctx = gpu
    batch = 5 if lg <= 12 else 3          # ragged batches: not a multiple of the tile's polynomial count
    x = rand_field(100 + lg, (batch, 1 << lg))
    f = p.fft(x)
    assert (f == orc.fft(x)).all()
    assert (p.ifft(x) == orc.ifft(x)).all()
    assert (p.ifft(f) == x).all()
    assert (p.coset_fft(x, 7) == orc.coset_fft(x, 7)).all()
    assert (p.coset_ifft(x, 7) == orc.coset_ifft(x, 7)).all()
    s = 0x123456789ABCDEF % P
    assert (p.coset_fft(x, s) == orc.coset_fft(x, s)).all()


@pytest.mark.parametrize("lg,rate", [(0, 3), (1, 3), (3, 3), (5, 1), (9, 3), (10, 3), (12, 3), (13, 2), (15, 3)])
def test_coset_lde_matches_oracle(gpu, orc, lg, rate):
    p, ctx = gpu
    x = rand_field(200 + lg, (3, 1 << lg))
    assert (p.lde_onto_coset(x, rate) == orc.lde(x, rate, threads=4)).all()


@pytest.mark.parametrize("lg,rate,batch", [(17, 3, 2), (11, 3, 7), (14, 3, 5), (16, 4, 4), (12, 2, 6)])
def test_coset_lde_batches_and_config2_shape(gpu, orc, lg, rate, batch):
    # BASELINE config 2's LDE shape (2^17 -> 2^20, coset 7, benches/ffts.rs:21-37) and batches of >= 4 polynomials, which
    # take the inter-pass twiddle table and (rate >= 8) the zero-padding-aware first stage of the column pass
    p, ctx = gpu
    x = rand_field(700 + lg, (batch, 1 << lg))
    assert (p.lde_onto_coset(x, rate) == orc.lde(x, rate, threads=8)).all()


def test_ntt_non_canonical_input(gpu, orc):
    p, ctx = gpu
    x = np.random.default_rng(7).integers(0, 2**64, size=(2, 1 << 13), dtype=np.uint64)
    assert (p.fft(x) == orc.fft(x)).all()
    assert (p.ifft(x) == orc.ifft(x)).all()


def test_ntt_extreme_values(gpu, orc):
    # inputs made only of the edge values (0, 1, 2^32 +- 1, p - 1, p, p + 1, 2^64 - 1): every carry / borrow correction of the
    # butterflies, shift twiddles and table multiplies, single-pass and two-pass sizes, plain, inverse and zero-padded coset LDE
    p, ctx = gpu
    edge = np.array([0, 1, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P, P + 1, 2**63, 2**64 - 2**32, 2**64 - 1], dtype=np.uint64)
    rng = np.random.default_rng(3)
    for lg in (4, 10, 13, 16):
        x = edge[rng.integers(0, len(edge), (5, 1 << lg))]
        x[0, :] = 2**64 - 1
        x[1, :] = P - 1
        assert (p.fft(x) == orc.fft(x)).all(), lg
        assert (p.ifft(x) == orc.ifft(x)).all(), lg
        if lg <= 13:
            assert (p.lde_onto_coset(x, 3) == orc.lde(x, 3, threads=4)).all(), lg


@pytest.mark.parametrize("lg", [4, 6, 8, 10, 12, 13, 16, 20])
def test_ntt_structured_inputs(gpu, orc, lg):
    # sparse and power-of-two columns: unit vectors, 2^k, h 2^(96-E), p - 2^k.  With such inputs a transform carries +-2^k through
    # its layers, which is where the shift twiddles take their rare paths (x 2^E with a zero low and middle word: the borrow
    # without carry of glx_shl_c, 32 < E < 64) that uniformly random columns reach with probability ~2^-32 per operation.
    # Closed forms besides the oracle: fft(e_j)[i] = w^(i j), and fft of a constant column is (n c, 0, 0, ...).
    p, ctx = gpu
    n = 1 << lg
    rng = np.random.default_rng(lg)
    rows = []
    for j in (0, 1, 2, n // 2, n - 1, int(rng.integers(0, n))):          # unit vectors (scaled by 1, 2^63, p - 1)
        for c in (1, 2**63, P - 1):
            v = np.zeros(n, dtype=np.uint64); v[j % n] = c; rows.append(v)
    pw = np.array([(1 << int(k)) % P for k in rng.integers(0, 64, n)], dtype=np.uint64)
    rows.append(pw)                                                          # every entry a power of two
    rows.append(np.array([P - (1 << int(k)) for k in rng.integers(0, 64, n)], dtype=np.uint64))
    hs = [(int(h) << (96 - E)) % 2**64 for E in (36, 48, 60) for h in (1, 3, 7, (1 << (E - 32)) - 1)]
    rows.append(np.array([hs[int(i)] for i in rng.integers(0, len(hs), n)], dtype=np.uint64))
    sp = np.zeros(n, dtype=np.uint64); sp[rng.integers(0, n, max(1, n // 64))] = 2**63; rows.append(sp)     # sparse
    rows.append(np.full(n, 2**63, dtype=np.uint64))                          # constant column
    x = np.stack(rows)
    f = p.fft(x)
    if lg <= 16:
        assert (f == orc.fft(x)).all()
        assert (p.ifft(x) == orc.ifft(x)).all()
        assert (p.coset_fft(x, 7) == orc.coset_fft(x, 7)).all()
    else:
        assert (f[:2] == orc.fft(x[:2])).all() and (f[-4:] == orc.fft(x[-4:])).all()
    assert (p.ifft(f) == x).all()
    assert ints(f[0]) == [1] * n                                            # e_0 -> all ones
    w = pow(7, (P - 1) >> lg, P) if lg else 1                               # the reference's primitive root of unity (fft.rs:14-33)
    assert pow(w, n, P) == 1
    if lg <= 12:
        assert ints(f[3]) == [pow(w, i, P) for i in range(n)]              # e_1 -> w^i
    assert int(f[-1][0]) == (n * 2**63) % P and not f[-1][1:].any()
    if 3 <= lg <= 13:
        assert (p.lde_onto_coset(x, 3) == orc.lde(x, 3, threads=4)).all()


def test_ntt_2_20_against_oracle_and_round_trip(gpu, orc):
    # BASELINE config 2: 2^20-point forward + inverse, bit-exact vs field::fft on B = 2; properties on B = 8
    p, ctx = gpu
    x = rand_field(20, (2, 1 << 20))
    f = p.fft(x)
    assert (f == orc.fft(x)).all()
    assert (p.ifft(f) == x).all()
    assert (p.ifft(x) == orc.ifft(x)).all()
    y = rand_field(21, (8, 1 << 20))
    fy = p.fft(y)
    assert (p.ifft(fy) == y).all()
    # linearity: fft(a) + fft(b) == fft(a + b)
    s = orc.field_op(0, y[0], y[1])
    assert (orc.field_op(0, fy[0], fy[1]) == p.fft(s)).all()
    # first output is the sum of the coefficients
    for b in range(2):
        assert int(fy[b][0]) == sum(int(v) for v in y[b]) % P


def test_ntt_large_sizes_round_trip(gpu, orc):
    p, ctx = gpu
    for lg in (17, 18, 19, 21, 22):
        x = rand_field(300 + lg, (2, 1 << lg))
        f = p.fft(x)
        assert (p.ifft(f) == x).all(), lg
        assert int(f[1][0]) == sum(int(v) for v in x[1]) % P
        if lg <= 18:
            assert (f == orc.fft(x)).all()


@pytest.mark.parametrize("lg", [19, 21])
def test_ntt_2_19_and_2_21_by_value_against_the_oracle(gpu, orc, lg):
    # the two two-pass sizes above 2^18 that the round trip above checks only against themselves: 2^21 is the m = 128 LDE size and the only
    # user of ntt_row_pass<11>.  Forward, inverse and coset forms on two columns, and at 2^21 the LDE from 2^18 with its zero padding.
    p, ctx = gpu
    x = rand_field(700 + lg, (2, 1 << lg))
    assert (p.fft(x) == orc.fft(x)).all()
    assert (p.ifft(x) == orc.ifft(x)).all()
    s = 0x123456789ABCDEF % P
    assert (p.coset_fft(x, s) == orc.coset_fft(x, s)).all()
    assert (p.coset_fft(x) == orc.coset_fft(x, 7)).all()
    if lg == 21:
        c = rand_field(750 + lg, (2, 1 << (lg - 3)))
        assert (p.lde_onto_coset(c, 3) == orc.lde(c, 3, threads=8)).all()


@pytest.mark.parametrize("lg", [22, 23, 24])
def test_ntt_three_pass_sizes_against_the_oracle(gpu, orc, lg):
    # from 2^22 points on the transform is nested: 2^9 / 2^10-point columns, then the M-point rows as a two-pass transform whose row pass
    # scatters into the result (ntt.hip gl_ntt_run).  Forward, inverse, coset forms, the LDE with its zero padding, a batch that needs
    # two chunks of the inter-pass scratch: all against the oracle's radix-2 transforms.
    p, ctx = gpu
    x = rand_field(900 + lg, (2, 1 << lg))
    f = p.fft(x)
    assert (f == orc.fft(x)).all()
    assert (p.ifft(f) == x).all()
    assert (p.ifft(x[:1]) == orc.ifft(x[:1])).all()
    s = 0x123456789ABCDEF % P
    assert (p.coset_fft(x[:1], s) == orc.coset_fft(x[:1], s)).all()
    assert (p.coset_ifft(x[:1], 7) == orc.coset_ifft(x[:1], 7)).all()
    c = rand_field(950 + lg, (2, 1 << (lg - 3)))
    assert (p.lde_onto_coset(c, 3) == orc.lde(c, 3, threads=8)).all()
    ctx.set_scratch_elems(1 << lg)                      # one polynomial per chunk
    try:
        y = rand_field(990 + lg, (3, 1 << lg))
        fy = p.fft(y)
        assert (fy[2] == orc.fft(y[2:3])[0]).all() and (fy[0] == p.fft(y[0:1])[0]).all()
    finally:
        ctx.set_scratch_elems(1 << 24)


def test_ntt_chunked_batches(gpu, orc):
    # more polynomials than fit the inter-pass scratch: exercises the chunk loop
    p, ctx = gpu
    ctx.set_scratch_elems(1 << 15)
    try:
        x = rand_field(77, (11, 1 << 14))
        assert (p.fft(x) == orc.fft(x)).all()
    finally:
        ctx.set_scratch_elems(1 << 24)


def test_ntt_table_cache_in_a_fresh_context_in_a_fixed_order_of_use(gpu, orc):
    # gl_ntt_run keeps its power tables per context (gl_ctx::get_pow_table): a table is created at the length of its first use, regrown
    # when a longer one is asked for (the short one is parked, it may be in flight) and reused when it is long enough.  One fixed order
    # of use in a context that has no table yet, every result against the oracle.
    p, _ = gpu
    ctx = p.Context(0)
    small, big, mid = rand_field(4100, (3, 1 << 10)), rand_field(4101, (2, 1 << 16)), rand_field(4102, (3, 1 << 12))
    lde_want = orc.lde(small, 3, threads=4)
    assert (p.lde_onto_coset(small, 3, ctx=ctx) == lde_want).all()                   # creates the short table of the shift 7
    assert (p.coset_fft(big, ctx=ctx) == orc.coset_fft(big)).all()                   # regrows it, parks the short one
    assert (p.lde_onto_coset(small, 3, ctx=ctx) == lde_want).all()                   # the longer table serves the short use
    assert (p.coset_fft(mid, ctx=ctx) == orc.coset_fft(mid)).all()
    for batch in (4, 5):                                                             # the pass table that carries the 1/N scale, made once
        v = rand_field(4103 + batch, (batch, 1 << 13))
        assert (p.ifft(v, ctx=ctx) == orc.ifft(v)).all()
    ctx.synchronize()


# --------------------------------------------------------------------------------------- Poseidon/Merkle
def test_poseidon_known_answers(gpu, orc, golden):
    p, ctx = gpu
    for kat in golden["poseidon_kats"] + golden["poseidon_model"]:
        assert ints(p.poseidon(np.array(kat["input"], dtype=np.uint64))) == kat["output"]
    r = np.random.default_rng(11).integers(0, 2**64, size=(4096, 12), dtype=np.uint64)
    assert (p.poseidon(r) == orc.poseidon(r)).all()


def test_poseidon_extreme_and_non_canonical_states(gpu, orc):
    # every carry / borrow path of the GPU permutation (32-bit-half MDS accumulators, the three-round groups, reduce96/128):
    # states built from the edge values 0, 1, 2^32-1, 2^32, p-1, p, p+1, 2^64-1 in all positions plus random mixes of them
    p, ctx = gpu
    edge = np.array([0, 1, 2**32 - 1, 2**32, 2**32 + 1, P - 1, P, P + 1, 2**63, 2**64 - 2**32, 2**64 - 1], dtype=np.uint64)
    rng = np.random.default_rng(12)
    states = [np.full(12, e, dtype=np.uint64) for e in edge]
    for _ in range(400):
        states.append(edge[rng.integers(0, len(edge), 12)])
    for k in range(12):
        st = np.zeros(12, dtype=np.uint64); st[k] = 2**64 - 1; states.append(st)
    states = np.stack(states)
    got, want = p.poseidon(states), orc.poseidon(states)
    assert (got == want).all()
    # the cooperative (16 lanes per state) and fused-top variants see the same values through tiny Merkle trees
    leaves = states[:256, :8].copy()
    for cap_height in (0, 4):
        assert (p.MerkleTree(leaves, cap_height).cap == orc.merkle(leaves, cap_height).cap).all()


@pytest.mark.parametrize("ln", [1, 3, 4, 5, 7, 8, 9, 16, 17, 32, 84, 135])
def test_hash_or_noop_rows(gpu, orc, ln):
    p, ctx = gpu
    rows = np.random.default_rng(ln).integers(0, 2**64, size=(33, ln), dtype=np.uint64)
    got = p.hash_or_noop(rows)
    for i in range(33):
        assert (got[i] == orc.hash_or_noop(rows[i])).all()


def test_merkle_tree_golden_and_oracle(gpu, orc, golden):
    p, ctx = gpu
    m = golden["merkle_model"]
    leaves = np.array(m["leaves"], dtype=np.uint64)
    for t in m["trees"]:
        tree = p.MerkleTree(leaves, t["cap_height"])
        assert tree.cap.tolist() == t["cap"]
        for idx, sib in t["paths"].items():
            assert tree.prove(int(idx)).tolist() == sib
    s = golden["merkle_short"]
    assert p.MerkleTree(np.array(s["leaves"], dtype=np.uint64), s["cap_height"]).cap.tolist() == s["cap"]
    # merkle_tree.rs:253-281: 256 x 7 random leaves, every path verifies to the cap, cap heights 1 and 8
    leaves = rand_field(9, (256, 7))
    for cap_height in (0, 1, 8):
        tree = p.MerkleTree(leaves, cap_height)
        ot = orc.merkle(leaves, cap_height)
        assert (tree.cap == ot.cap).all()
        for i in range(0, 256, 5):
            sib = tree.prove(i)
            assert (sib == ot.prove(i)).all()
            assert orc.merkle_verify(leaves[i], i, tree.cap, sib)
    with pytest.raises(p.Plonky2Mi355xError):
        p.MerkleTree(leaves, 9)        # merkle_tree.rs:137-143
    # one-leaf tree and single-element leaves
    one = rand_field(10, (1, 5))
    assert (p.MerkleTree(one, 0).cap == orc.merkle(one, 0).cap).all()


@pytest.mark.parametrize("lg", [0, 1, 2, 3, 5, 7, 9, 10, 11, 12, 13, 14, 15])
def test_merkle_shapes_across_kernel_paths(gpu, orc, lg):
    # tree shapes on both sides of every kernel switch: one hash per lane / 16 lanes per hash (<= 8192 hashes), and the
    # single-launch tree top (levels with <= 64 nodes per cap subtree), for cap heights 0..5 and short / long leaves
    p, ctx = gpu
    n = 1 << lg
    for leaf_len in (1, 4, 5, 8, 32):
        leaves = rand_field(5000 + 10 * lg + leaf_len, (n, leaf_len))
        for cap_height in sorted({0, 1, 4, 5, lg} & set(range(lg + 1))):
            tree = p.MerkleTree(leaves, cap_height)
            ot = orc.merkle(leaves, cap_height)
            assert (tree.cap == ot.cap).all(), (lg, leaf_len, cap_height)
            for i in sorted({0, n // 3, n - 1}):
                sib = tree.prove(i)
                assert (sib == ot.prove(i)).all(), (lg, leaf_len, cap_height, i)


# -------------------------------------------------------------------------------------- PolynomialBatch
def test_polynomial_batch_golden(gpu, golden):
    p, ctx = gpu
    m = golden["batch_model"]
    b = p.PolynomialBatch.from_values(np.array(m["values"], dtype=np.uint64), m["rate_bits"], False, m["cap_height"])
    assert b.polynomials.tolist() == m["coeffs"]
    assert b.lde_values().tolist() == m["lde"]
    assert b.cap.tolist() == m["cap"]
    assert b.get_leaf(13).tolist() == m["leaf_13"]
    m9 = golden["batch_model9"]
    b9 = p.PolynomialBatch.from_values(np.array(m9["values"], dtype=np.uint64), m9["rate_bits"], False, m9["cap_height"])
    assert b9.cap.tolist() == m9["cap"]
    assert b9.prove(37).tolist() == m9["path_37"]
    with pytest.raises(p.Plonky2Mi355xError):
        p.PolynomialBatch.from_values(np.array(m["values"], dtype=np.uint64), 3, True, 2)   # blinding unsupported


@pytest.mark.parametrize("ncols,lg,rate,cap", [(1, 3, 3, 4), (3, 0, 3, 2), (4, 5, 3, 4), (20, 10, 3, 4), (135, 12, 3, 4), (16, 13, 3, 4)])
def test_polynomial_batch_matches_oracle(gpu, orc, ncols, lg, rate, cap):
    p, ctx = gpu
    vals = rand_field(500 + ncols, (ncols, 1 << lg))
    for from_values in (True, False):
        ob = orc.batch(vals, rate, cap, from_values=from_values, threads=8)
        gb = (p.PolynomialBatch.from_values if from_values else p.PolynomialBatch.from_coeffs)(vals, rate, False, cap)
        assert (gb.polynomials == ob.polynomials).all()
        assert (gb.cap == ob.cap).all()
        N = 1 << (lg + rate)
        lde = gb.lde_values()
        for j in sorted({0, 1, N // 3, N - 1}):
            leaf = gb.get_leaf(j)
            assert (leaf == ob.get_leaf(j)).all()
            sib = gb.prove(j)
            assert (sib == ob.prove(j)).all()
            assert orc.merkle_verify(leaf, j, gb.cap, sib)
            rev = int(format(j, "0%db" % (lg + rate))[::-1], 2) if lg + rate else 0
            assert (lde[:, rev] == leaf).all()
            assert (gb.get_lde_values(rev, 1) == leaf).all()      # oracle.rs:128-133
        gb.free()


# ---------------------------------------------------------------------------------------------------- prove()
def _prove_both(p, orc, m, seed, threads=8):
    hc = p.MatmulCircuit(m)
    oc = orc.circuit(m, threads=threads)
    a, b = rand_field(seed, m * m) % (2**32 - 1), rand_field(seed + 1, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=seed)
    cd = hc.build()
    assert (cd.constants_sigmas_cap == oc.constants_sigmas_cap).all()
    assert (cd.circuit_digest == oc.digest).all()
    gp = cd.prove(wires, pis)
    op = oc.witness(a, b, filler_seed=seed).prove(threads=threads)
    return gp, op


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 20])
def test_prove_is_byte_identical_to_the_oracle(gpu, orc, m):
    # BASELINE configs[0] (m = 2, README instance shape) and sizes with 0, 1 and 2 FRI reduction rounds
    p, ctx = gpu
    gp, op = _prove_both(p, orc, m, 1000 + m)
    assert gp.challenges() == op.challenges()
    assert (gp.caps() == op.caps()).all()
    assert (gp.zs_partial_products() == op.zs_partial_products()).all()
    assert (gp.quotient_chunks() == op.quotient_chunks()).all()
    assert gp.query_indices() == op.query_indices()
    assert gp.to_bytes() == op.to_bytes()
    assert op.verify()[0]                      # ... and the native verifier restatement accepts those bytes' proof


def test_prove_full_range_operands_and_edge_values(gpu, orc):
    # matrix entries over the whole field (the demo draws u32) and made of edge values: more carry paths in the permutation
    # argument, the quotient and FRI; still byte-identical to the oracle
    p, ctx = gpu
    m = 8
    hc, oc = p.MatmulCircuit(m), orc.circuit(m, threads=8)
    cd = hc.build()
    edge = np.array([0, 1, 2**32 - 1, 2**32, P - 1, P - 2, 2**63, (P - 1) // 2], dtype=np.uint64)
    rng = np.random.default_rng(8)
    for a, b in ((rand_field(801, m * m), rand_field(802, m * m)), (edge[rng.integers(0, len(edge), m * m)], edge[rng.integers(0, len(edge), m * m)])):
        wires, pis = hc.witness(a, b, filler_seed=5)
        ow = oc.witness(a, b, filler_seed=5)
        assert (ow.wires() == wires).all()
        gp, op = cd.prove(wires, pis), ow.prove(threads=8)
        assert gp.to_bytes() == op.to_bytes()
        assert cd.verify(gp) == (True, "")


def test_prove_readme_instance(gpu, orc):
    p, ctx = gpu
    hc = p.MatmulCircuit(2)
    wires, pis = hc.witness([1, 2, 3, 4], [5, 6, 7, 8])
    assert pis.reshape(-1, 3)[:, 2].tolist() == [19, 22, 43, 50]
    proof = hc.build().prove(wires, pis)
    op = orc.circuit(2).witness([1, 2, 3, 4], [5, 6, 7, 8]).prove()
    assert proof.to_bytes() == op.to_bytes() and len(proof.to_bytes()) == 70288
    with pytest.raises(p.Plonky2Mi355xError):
        hc.build().prove(wires, pis[:-1])      # wrong number of public inputs
    # the witness as 135 separate host vectors (MatrixWitness.wire_values)
    cols = [wires[c].copy() for c in range(135)]
    assert hc.build().prove_columns(cols, pis).to_bytes() == op.to_bytes()


def test_prove_m64_matches_oracle(gpu, orc):
    # BASELINE configs[2]: m = 64, n = 2^15, three arity-16 FRI rounds; ~250 KB proof
    p, ctx = gpu
    gp, op = _prove_both(p, orc, 64, 64, threads=16)
    assert gp.challenges() == op.challenges()
    assert (gp.caps() == op.caps()).all()
    gb = gp.to_bytes()
    assert gb == op.to_bytes() and len(gb) == 250756
    assert op.verify()[0]
    hc = p.MatmulCircuit(64)
    assert hc.verify(gb, op.c.constants_sigmas_cap, op.c.digest) == (True, "")        # the product's own verify()


def test_oracle_verifier_accepts_gpu_proof_bytes(gpu, orc):
    # the restated native verifier (plonk/verifier.rs:15-115) parses the GPU's ProofWithPublicInputs bytes and accepts them,
    # given only VerifierOnlyCircuitData (cap, digest) produced by the GPU build; tampered bytes are rejected
    p, ctx = gpu
    for m in (2, 8, 20):
        hc = p.MatmulCircuit(m)
        a, b = rand_field(3 * m, m * m) % (2**32 - 1), rand_field(3 * m + 1, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=m)
        cd = hc.build()
        by = cd.prove(wires, pis).to_bytes()
        v = orc.circuit(m, verifier_only=True)
        ok, msg = v.verify_bytes(by, cd.constants_sigmas_cap, cd.circuit_digest)
        assert ok, msg
        bad = bytearray(by)
        bad[len(by) // 2] ^= 0x40
        assert not v.verify_bytes(bytes(bad), cd.constants_sigmas_cap, cd.circuit_digest)[0]
        assert not v.verify_bytes(by, cd.constants_sigmas_cap, cd.circuit_digest ^ np.uint64(1))[0]


def test_prove_m128_config5(gpu, orc):
    # BASELINE configs[4]: m = 128, n = 2^18, LDE 2^21, four arity-16 FRI rounds.  Too large for the CPU prover in a test;
    # parity is by properties: the restated native verifier accepts the GPU's bytes, proving twice gives identical bytes,
    # and the committed quotient really is the split of a degree-< 8n polynomial (checked through verification).
    p, ctx = gpu
    m = 128
    hc = p.MatmulCircuit(m)
    assert hc.degree_bits == 18 and hc.desc.num_fri_rounds == 4
    rng = np.random.default_rng(128)
    a = rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)
    b = rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)
    wires, pis = hc.witness(a, b, filler_seed=128)
    # spot-check the witness: C[5][7]
    c57 = sum(int(a[5 * m + k]) * int(b[k * m + 7]) for k in range(m)) % P
    assert int(pis[3 * (5 * m + 7) + 2]) == c57
    cd = hc.build()
    pr = cd.prove(wires, pis)
    by = pr.to_bytes()
    assert by == cd.prove(wires, pis).to_bytes()
    v = orc.circuit(m, verifier_only=True)
    ok, msg = v.verify_bytes(by, cd.constants_sigmas_cap, cd.circuit_digest)
    assert ok, msg
    assert cd.verify(pr) == (True, "")
    assert len(pr.challenges()["fri_betas"]) == 4


def test_warm_up_leaves_proofs_unchanged_and_takes_the_one_time_costs(gpu, orc):
    # gl_circuit_warm_up: a throw-away pass of the pipeline on a zero witness (which does not satisfy the circuit: nothing asserts it).
    # On a FRESH context the proof after it equals the proof without it byte for byte; for a lookup circuit too.
    import time
    p, ctx = gpu
    m = 32
    hc = p.MatmulCircuit(m)
    a, b = rand_field(1, m * m) % (2**32 - 1), rand_field(2, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=3)
    want = hc.build(ctx).prove(wires, pis).to_bytes()
    c2 = p.Context(device=0)
    cd2 = hc.build(c2).warm_up()
    t0 = time.perf_counter(); got = cd2.prove(wires, pis).to_bytes(); t_first = time.perf_counter() - t0
    t0 = time.perf_counter(); again = cd2.prove(wires, pis).to_bytes(); t_second = time.perf_counter() - t0
    assert got == want and again == want
    assert t_first < 3 * t_second + 0.005, (t_first, t_second)          # the first proof is no longer the slow one
    oc = orc.circuit_of_kind(10, 2, threads=8)
    w = oc.witness(np.array([3, 200, 17, 255], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=5)
    cd3 = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas(), ctx=p.Context(device=0)).warm_up()
    assert cd3.prove(w.wires(), w.public_inputs()).to_bytes() == w.prove(threads=8).to_bytes()


def test_prove_m256_the_largest_size_the_abi_takes(gpu):
    # m = 256: n = 2^21 rows, LDE 2^24 = the ABI's limit (degree_bits + rate_bits <= 24; two-pass NTT of 2^12 x 2^12 with tiles that span
    # several waves, 2.3 GB of witness through the pinned H2D ring, four arity-16 FRI rounds down to a 32-coefficient final polynomial, 1.77 MB proof).  No CPU prover at this size:
    # the native verifier accepts the bytes, rejects a flipped one, the witness spot-checks against the product of the matrices.
    p, ctx = gpu
    m = 256
    hc = p.MatmulCircuit(m)
    assert hc.degree_bits == 21 and hc.desc.num_fri_rounds == 4
    rng = np.random.default_rng(256)
    a = rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)
    b = rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)
    wires, pis = hc.witness(a, b, filler_seed=256)
    c = sum(int(a[200 * m + k]) * int(b[k * m + 31]) for k in range(m)) % P
    assert int(pis[3 * (200 * m + 31) + 2]) == c
    cd = hc.build()
    pr = cd.prove(wires, pis)
    by = pr.to_bytes()
    assert len(by) == 1774624 and cd.verify(pr) == (True, "")
    bad = bytearray(by); bad[len(by) // 2] ^= 4
    assert not cd.verify(bytes(bad))[0]
    assert len(pr.challenges()["fri_betas"]) == 4


# ------------------------------------------------------------------------------- phase-level ABI (SURVEY 8b seam)
@pytest.mark.parametrize("m,own", [(2, False), (8, False), (20, False), (8, True), (20, True)])
def test_phase_api_with_external_transcript_reproduces_the_proof(gpu, orc, m, own):
    # the phase entry points driven by a caller-side Challenger (the model, or the library's own): the assembled ProofWithPublicInputs
    # bytes equal the oracle's (and gl_prove's)
    p, ctx = gpu
    hc = p.MatmulCircuit(m)
    a, b = rand_field(7000 + m, m * m) % (2**32 - 1), rand_field(7001 + m, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=m)
    cd = hc.build()
    op = orc.circuit(m, threads=8).witness(a, b, filler_seed=m).prove(threads=8)

    r = drive_phase_api(p, ctx, orc, cd, LibraryChallenger(p) if own else poseidon_challenger(orc), wires, pis)
    assert (r.d_wires.download(wires.shape) == wires).all()            # the witness matrix is left untouched
    assert (r.q_b.polynomials == op.quotient_chunks()).all()
    assert (r.zs_b.open_at(r.zeta, 2, 18) == r.openings["pp"]).all()
    with pytest.raises(p.Plonky2Mi355xError):
        cd.fri(r.batches, r.zeta, r.fri_alpha).fold([1, 0])                # fold before commit
    with pytest.raises(p.Plonky2Mi355xError):
        r.fri.commit_round()                                                # no round left
    ob = op.to_bytes()
    assert len(r.bytes) == len(ob)
    assert r.bytes == ob
    assert r.bytes == cd.prove(wires, pis).to_bytes()
    assert op.challenges()["pow_witness"] == r.pow_witness and op.query_indices() == r.x_index


# ------------------------------------------------------------------------------- witness generation in HBM
@pytest.mark.parametrize("m", [1, 2, 3, 5, 20, 64])
def test_device_witness_generation_equals_host(gpu, orc, m):
    p, ctx = gpu
    hc = p.MatmulCircuit(m)
    gen = hc.witness_generator()
    buf = ctx.alloc(135 * hc.n * 8)
    for seed in (m, m + 100):
        a, b = rand_field(9000 + seed, m * m), rand_field(9500 + seed, m * m)       # full-range field elements, incl. > 2^32
        if seed == m:
            a[0], b[-1] = P - 1, P + 5 if m > 1 else 3                               # non-canonical input is canonicalised
        wires, pis = hc.witness(a, b, filler_seed=seed)
        buf.upload(np.full((135, hc.n), 0xDEADBEEF, dtype=np.uint64))               # stale contents must be overwritten
        dpis = gen.run(a, b, buf.ptr, filler_seed=seed)
        assert (dpis == pis).all()
        assert (buf.download((135, hc.n)) == wires).all()
    # ... and it proves: same bytes as proving the host witness
    if m in (2, 20):
        cd = hc.build()
        assert (gen.public_inputs_hash == orc.hash_no_pad(pis)).all()
        want = cd.prove(wires, pis).to_bytes()
        assert cd.prove_device(buf.ptr, dpis).to_bytes() == want
        assert cd.prove_device(buf.ptr, dpis, gen.public_inputs_hash).to_bytes() == want


def test_demo_binary_builds_proves_and_verifies(gpu):
    # examples/matrix_mul: the reference's bin/matrix_mul.rs flow (build, prove, print, verify) in C++ over the C ABI
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "matrix_mul")
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])      # a no-op when up to date; a binary built against an
    # older header (gl_circuit_desc grew in round 3) must never run: it hands the library a too-small struct
    for m, seed in ((2, 7), (20, 11)):
        r = subprocess.run([exe, str(m), str(seed)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip() == "length of proof.public_inputs is %d" % (3 * m * m)      # matrix_mul.rs:90
        assert "accepted" in r.stderr
    r = subprocess.run([exe, "20", "5", "9"], capture_output=True, text=True, timeout=300)   # + a batch of 9 through the pool
    assert r.returncode == 0 and "all accepted" in r.stderr, r.stderr


def test_hand_scheduled_primitives_against_int128(gpu):
    # tools/ubench/wide_acc.hip: the quotient's unreduced alpha-weighted sums (GlxWideAcc2), the 7 y = 8 y - y step and the
    # canonical factor chains of the permutation argument, each against unsigned __int128 arithmetic on the host
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "ubench", "bin", "wide_acc")
    src = os.path.join(root, "tools", "ubench", "wide_acc.hip")
    hdr = os.path.join(root, "plonky2_demo_amd", "csrc", "gl64_gfx950.cuh")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(root, "plonky2_demo_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 3, r.stdout


def test_goldilocks_primitives_edge_grid_against_int128(gpu):
    # tools/ubench/gl_prims.hip, the cost bench of the primitives, checks each CANDIDATE it times first.  From gl64_gfx950.cuh those are
    # glx_mul3<false / true> and glx_shl_c<12, 24, 32, 36, 48, 60, 72, 84> (one exponent or more per branch); the single product, add_cc /
    # sub_cc, the accumulator folds and the canonical fix-up it checks are its own look-alikes (m_mul_t, m_add_cc, m_sub_cc, m_accred,
    # m_reduce96, m_fix_canon), not the header's functions -- those are checked by tools/ubench/glx_check.hip (test_glx_primitives.py).
    # Inputs: an edge grid that holds the boundary forms of each branch (2^k for all k, p - 2^k, h 2^(96-E), low bits zero) x itself plus
    # random words, against unsigned __int128 on the host.  (this program was outside pytest, and
    # profiles/r02_gl_primitives.txt held FAIL rows of a development build of the 32 < E < 64 branch.)
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "ubench", "bin", "gl_prims")
    src = os.path.join(root, "tools", "ubench", "gl_prims.hip")
    hdr = os.path.join(root, "plonky2_demo_amd", "csrc", "gl64_gfx950.cuh")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-w", "-I", os.path.join(root, "plonky2_demo_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and "MISMATCH" not in r.stdout and "total mismatches: 0" in r.stdout, r.stdout


def test_concurrent_proofs_on_shared_circuit_are_deterministic(gpu):
    # four contexts (streams) of one device prove against ONE device-resident circuit from four host threads, as bench.py
    # does: every proof must equal the single-stream proof of the same witness byte for byte (no cross-stream state)
    import ctypes, threading
    p, ctx = gpu
    m = 20
    hc = p.MatmulCircuit(m)
    cd = hc.build(ctx)
    wits = []
    for k in range(3):
        a, b = rand_field(300 + k, m * m) % (2**32 - 1), rand_field(400 + k, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=k)
        wits.append((ctx.alloc(wires.nbytes).upload(wires), pis, cd.prove(wires, pis).to_bytes()))
    lanes = [(ctx, cd)] + [(lambda c: (c, p.api.CircuitView(cd, c)))(p.Context(device=0)) for _ in range(3)]
    results, errors = {}, []

    def work(lane):
        try:
            for rep in range(4):
                for k, (buf, pis, _) in enumerate(wits):
                    results[(lane, rep, k)] = lanes[lane][1].prove_device(buf.ptr, pis).to_bytes()
            lanes[lane][0].synchronize()
        except Exception as e:          # surfaced below: an assertion inside a thread would be lost
            errors.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors
    assert len(results) == 4 * 4 * 3
    for (lane, rep, k), by in results.items():
        assert by == wits[k][2], (lane, rep, k)


def test_concurrent_proofs_of_a_circuit_with_lookups_on_six_lanes(gpu, orc):
    # the all-gates circuit (two lookup tables, exponentiation, range check, ...; its own launches: k_lookup_inverses / k_lookup_scan per
    # table, k_quotient_lookup) proved from six host threads on six contexts against ONE device-resident circuit, from HOST wire matrices
    # (the pinned H2D ring per context): every proof equals the oracle's bytes for its witness
    import threading
    p, ctx = gpu
    oc = orc.circuit_of_kind(15, 9, threads=8)
    cd = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas())
    wits = []
    for k, (x, y) in enumerate(((200, 300), (0, 0), (255, 511))):
        w = oc.witness(np.array([x, y], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=k)
        wits.append((w.wires(), w.public_inputs(), w.prove(threads=8).to_bytes()))
    lanes = [p.api.CircuitView(cd, ctx)] + [p.api.CircuitView(cd, p.Context(device=0)) for _ in range(5)]
    results, errors = {}, []

    def work(lane):
        try:
            for rep in range(3):
                for k, (wires, pis, _) in enumerate(wits):
                    results[(lane, rep, k)] = lanes[lane].prove(wires, pis).to_bytes()
        except Exception as e:
            errors.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors
    assert len(results) == 6 * 3 * 3
    for (lane, rep, k), by in results.items():
        assert by == wits[k][2], (lane, rep, k)


def test_generic_prover_pool_proves_a_batch_of_host_witnesses(gpu, orc):
    # gl_prover_pool_create_generic / gl_prover_pool_prove_columns: six warmed-up lanes inside the library for the all-gates circuit and for
    # a Merkle-proof circuit; a batch of 20 host witnesses (135 separate column vectors each) in one call; every proof == the oracle's
    from test_verifier import merkle_proof_circuit_inputs
    p, ctx = gpu
    oc = orc.circuit_of_kind(15, 9, threads=8)
    pool = p.api.GenericProverPool(oc.product_desc(), oc.constants_sigmas(), lanes=6)
    wits, want = [], []
    for k in range(20):
        w = oc.witness(np.array([(37 * k) % 256, (91 * k) % 512], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=k)
        wires = w.wires()
        wits.append(([wires[j].copy() for j in range(135)], w.public_inputs()))
        want.append(w.prove(threads=8).to_bytes())
    got = pool.prove_columns(wits)
    assert [g.to_bytes() for g in got] == want
    assert pool.prove_columns([]) == []
    from plonky2_demo_amd._lib import lib, check
    with pytest.raises(p.Plonky2Mi355xError):
        check(lib.gl_prover_pool_prove_matmul(pool.handle, 0, None, None, None, None))      # a generic pool has no matmul witness generators
    pool.close()
    oc2 = orc.circuit_of_kind(14, 6, threads=8)
    pool2 = p.api.GenericProverPool(oc2.product_desc(), oc2.constants_sigmas(), lanes=3)
    wits, want = [], []
    for idx in (0, 21, 63, 42):
        a, _root = merkle_proof_circuit_inputs(orc, 6, idx)
        w = oc2.witness(a, np.zeros(0, dtype=np.uint64), filler_seed=idx)
        wits.append((w.wires(), w.public_inputs()))
        want.append(w.prove(threads=8).to_bytes())
    assert [g.to_bytes() for g in pool2.prove_columns(wits)] == want
    pool2.close()


def test_prover_pool_returns_the_first_error_and_keeps_the_proofs_already_made(gpu, orc):
    # the contract of the pools' lane runner (csrc/lanes.hpp), through gl_prover_pool_prove_columns itself: 3 lanes, 5 items of which
    # item 3 has no witness -> the status and text of that item, every proof that was produced is the oracle's, item 3 stays null,
    # and the pool proves a good batch afterwards
    import ctypes
    from plonky2_demo_amd._lib import lib, GL_OK, ERRORS
    p, ctx = gpu
    m = 2
    hc, oc = p.MatmulCircuit(m), orc.circuit(m, threads=4)
    pool = p.api.GenericProverPool(hc.desc, hc.constants_sigmas(), lanes=3)
    cols, pis, want = [], [], []
    for k in range(5):
        a, b = rand_field(300 + k, m * m) % (2**32 - 1), rand_field(400 + k, m * m) % (2**32 - 1)
        w = oc.witness(a, b, filler_seed=k)
        wires = w.wires()
        cols.append([np.ascontiguousarray(wires[j]) for j in range(135)])
        pis.append(np.ascontiguousarray(w.public_inputs()))
        want.append(w.prove(threads=4).to_bytes())
    col_arrays = [(ctypes.c_void_p * 135)(*[c.ctypes.data for c in item]) for item in cols]

    def prove(null_item):
        col_ptrs = (ctypes.c_void_p * 5)(*[None if i == null_item else ctypes.addressof(col_arrays[i]) for i in range(5)])
        pi_ptrs = (ctypes.c_void_p * 5)(*[v.ctypes.data for v in pis])
        out = (ctypes.c_void_p * 5)()
        st = lib.gl_prover_pool_prove_columns(pool.handle, 5, col_ptrs, pi_ptrs, out)
        text = (lib.gl_last_error() or b"").decode()
        return st, text, [p.api.Proof(out[i], hc.desc).to_bytes() if out[i] else None for i in range(5)]

    st, text, got = prove(3)
    assert ERRORS.get(st) == "GL_ERR_ARG" and "null witness" in text, (st, text)
    assert got[3] is None
    for i in range(5):
        assert got[i] is None or got[i] == want[i], i
    st, text, got = prove(None)
    assert st == GL_OK, text
    assert got == want
    pool.close()


def test_host_witness_entry_on_eight_lanes_equals_prove_device(gpu):
    # the drop-in entry (plonk/prover.rs:145 -> gl_prove_columns): 64 proofs of the m = 64 circuit from HOST
    # witness matrices -- 135 separate pageable vectors each, as MatrixWitness.wire_values holds them (iop/witness.rs:256-258) -- on 8
    # lanes at once, each through the library's two-deep pinned H2D ring, byte-identical to gl_prove_device of the same witness; the
    # chunked copy is also exercised with columns that straddle chunk boundaries (m = 20: 8 KiB columns, one chunk)
    import threading
    p, ctx = gpu
    for m, count, nl in ((64, 64, 8), (20, 12, 4)):
        hc = p.MatmulCircuit(m)
        cd = hc.build(ctx)
        wits = []
        for k in range(4):
            a, b = rand_field(900 + k, m * m) % (2**32 - 1), rand_field(950 + k, m * m) % (2**32 - 1)
            wires, pis = hc.witness(a, b, filler_seed=70 + k)
            dbuf = ctx.alloc(wires.nbytes).upload(wires)              # (kept alive across the call: the proof reads it)
            want = cd.prove_device(dbuf.ptr, pis).to_bytes()
            dbuf.free()
            cols = p.api.HostColumns([wires[c].copy() for c in range(135)], hc.n)      # 135 separate allocations
            wits.append((cols, pis, want, wires))
        lanes = [(ctx, cd)] + [(lambda c: (c, p.api.CircuitView(cd, c)))(p.Context(device=0)) for _ in range(nl - 1)]
        out, errors = [None] * count, []

        def work(lane):
            try:
                for i in range(lane, count, nl):
                    out[i] = lanes[lane][1].prove_columns(wits[i % 4][0], wits[i % 4][1]).to_bytes()
                lanes[lane][0].synchronize()
            except Exception as e:
                errors.append(e)
        ths = [threading.Thread(target=work, args=(k,)) for k in range(nl)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        assert not errors, errors
        for i in range(count):
            assert out[i] == wits[i % 4][2], (m, i)
        # the contiguous-matrix entry (gl_prove) goes through the same ring
        assert cd.prove(wits[1][3], wits[1][1]).to_bytes() == wits[1][2]
        ok, why = cd.verify(out[0])
        assert ok, why


def test_sixteen_proofs_in_flight_m64_soak(gpu):
    # bench.py's configuration: 16 contexts, the first of them the circuit's own, 16 host threads, m = 64 -- and, as tools/soak.py
    # does, every thread now and then verifies a proof, which reads the circuit's Merkle cap through the CIRCUIT's context while
    # that context is proving on another thread (round 2: a single pinned staging buffer per context corrupted one proof in
    # 40-250 this way, while the 4-lane m = 20 test above stayed green).  Every proof must equal the single-stream proof of
    # its witness.
    import hashlib, threading
    p, ctx = gpu
    m, nl, per_lane = 64, 16, 24
    hc = p.MatmulCircuit(m)
    cd = hc.build(ctx)
    wits = []
    for k in range(5):
        a, b = rand_field(700 + k, m * m) % (2**32 - 1), rand_field(800 + k, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=k)
        buf = ctx.alloc(wires.nbytes).upload(wires)
        ref = cd.prove_device(buf.ptr, pis).to_bytes()
        assert cd.verify(ref) == (True, "")
        wits.append((buf, pis, hashlib.sha256(ref).digest()))
    lanes = [(ctx, cd)] + [(lambda c: (c, p.api.CircuitView(cd, c)))(p.Context(device=0)) for _ in range(nl - 1)]
    bad, errors = [], []

    def work(lane):
        try:
            for rep in range(per_lane):
                k = (lane + rep) % len(wits)
                by = lanes[lane][1].prove_device(wits[k][0].ptr, wits[k][1]).to_bytes()
                if hashlib.sha256(by).digest() != wits[k][2]:
                    bad.append((lane, rep, k))
                elif (lane + rep) % 5 == 0 and cd.verify(by) != (True, ""):    # reads the circuit's cap through the circuit's context
                    bad.append((lane, rep, k, "rejected"))
            lanes[lane][0].synchronize()
        except Exception as e:
            errors.append((lane, e))

    ths = [threading.Thread(target=work, args=(i,)) for i in range(nl)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors
    assert not bad, bad


def test_phase_api_rejects_mismatched_arguments(gpu):
    # the reference asserts on shape errors (oracle.rs:114,169); the phase entry points return GL_ERR_ARG instead
    p, ctx = gpu
    hc8, hc20 = p.MatmulCircuit(8), p.MatmulCircuit(20)
    cd8, cd20 = hc8.build(), hc20.build()
    a, b = rand_field(1, 64) % (2**32 - 1), rand_field(2, 64) % (2**32 - 1)
    wires, pis = hc8.witness(a, b)
    d_w = ctx.alloc(wires.nbytes).upload(wires)
    wb = p.PolynomialBatch.from_device(d_w.ptr, 135, hc8.n, 3, 4, True)
    zs = cd8.partial_products(d_w.ptr, [3, 5], [7, 11])
    assert zs.ncols == 20 and zs.degree == hc8.n
    with pytest.raises(p.Plonky2Mi355xError):
        cd20.quotient_polys(wb, zs, [1, 2, 3, 4], [3, 5], [7, 11], [13, 17])       # batches of another circuit size
    with pytest.raises(p.Plonky2Mi355xError):
        cd8.quotient_polys(zs, wb, [1, 2, 3, 4], [3, 5], [7, 11], [13, 17])        # wires / Z batches swapped
    q = cd8.quotient_polys(wb, zs, [1, 2, 3, 4], [3, 5], [7, 11], [13, 17])
    with pytest.raises(p.Plonky2Mi355xError):
        cd8.fri([wb, cd8.constants_sigmas_batch, zs, q], [2, 3], [5, 7])            # wrong oracle order
    with pytest.raises(p.Plonky2Mi355xError):
        wb.open_at([1, 2], first_col=130, num_cols=10)                              # column range out of bounds
    with pytest.raises(p.Plonky2Mi355xError):
        p.pow_grind(np.zeros(12, dtype=np.uint64), np.zeros(8, dtype=np.uint64), 16)   # no room for the witness in the rate
    fri = cd8.fri([cd8.constants_sigmas_batch, wb, zs, q], [2, 3], [5, 7])
    with pytest.raises(p.Plonky2Mi355xError):
        fri.final_poly()                                                              # reduction rounds not finished
    with pytest.raises(p.Plonky2Mi355xError):
        fri.query([0])


def test_gpu_proof_regression_hashes(gpu):
    # the same recorded SHA-256 values (tests/golden/proof_hashes.json), from the GPU prover alone: no oracle in the loop
    import hashlib, json, os
    p, ctx = gpu
    want = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "proof_hashes.json")))
    hc = p.MatmulCircuit(2)
    wires, pis = hc.witness([1, 2, 3, 4], [5, 6, 7, 8])
    assert hashlib.sha256(hc.build().prove(wires, pis).to_bytes()).hexdigest() == want["readme_m2"]
    for m, seed in ((1, 11), (3, 12), (8, 13), (20, 14)):
        hc = p.MatmulCircuit(m)
        a, b = rand_field(seed, m * m) % (2**32 - 1), rand_field(seed + 100, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=seed)
        cd = hc.build()
        w = want["m%d_seed%d" % (m, seed)]
        assert [int(x) for x in cd.circuit_digest] == w["digest"]
        pr = cd.prove(wires, pis)
        assert pr.challenges()["pow_witness"] == w["pow_witness"]
        assert hashlib.sha256(pr.to_bytes()).hexdigest() == w["sha256"]
        assert cd.verify(pr) == (True, "")


@pytest.mark.parametrize("kind,param", [(1, 16), (1, 5), (1, 40), (1, 4000), (2, 50), (2, 400), (2, 3000), (2, 200000)])
def test_generic_circuits_over_the_same_gate_set(gpu, orc, kind, param):
    # gl_circuit_create + gl_prove are not tied to the matmul layout: circuits built by the oracle's generic CircuitBuilder with
    # other gate subsets (no ArithmeticGate / no PoseidonGate and zero public inputs / no NoopGate), one or two selector groups
    p, ctx = gpu
    oc = orc.circuit_of_kind(kind, param, threads=8)
    a = rand_field(100 * kind + param, param if kind == 1 else 2)
    w = oc.witness(a, np.zeros(0, dtype=np.uint64), filler_seed=kind)
    _prove_generic_and_compare(p, oc, w)


def _prove_generic_and_compare(p, oc, w):
    op = w.prove(threads=8)
    cd = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas())
    assert (cd.circuit_digest == oc.digest).all() and (cd.constants_sigmas_cap == oc.constants_sigmas_cap).all()
    gp = cd.prove(w.wires(), w.public_inputs())
    assert gp.challenges() == op.challenges()
    assert gp.to_bytes() == op.to_bytes()
    assert cd.verify(gp) == (True, "")
    assert oc.verify_bytes(gp.to_bytes(), cd.constants_sigmas_cap, cd.circuit_digest)[0]
    return gp


@pytest.mark.parametrize("name,kind,param,inputs,outputs", [
    ("fibonacci", 3, 99, [0, 1], [0, 1, 3736710860384812976]),        # examples/fibonacci.rs:22-42 (the README's printed value)
    ("fibonacci from (5, 8)", 3, 99, [5, 8], None),
    ("factorial", 4, 100, [1], [1, 3822706312645553057]),              # examples/factorial.rs:22-36
    ("easy polynomial", 5, 0, [1], [1, 4]),                            # examples/easy_polynomial.rs:19-31: x^2 - 4x + 7 at 1
    ("easy polynomial at p - 3", 5, 0, [P - 3], [P - 3, 28]),
    ("square root", 6, 0, [1234567890123456789], [1234567890123456789 ** 2 % P]),     # examples/square_root.rs:104-107
])
def test_reference_example_circuits(gpu, orc, name, kind, param, inputs, outputs):
    # the reference's own example programs that use only the five supported gates, built by the oracle's generic CircuitBuilder
    # (several ConstantGates, the arithmetic memo table, 2-8 rows ... 64 rows), proved on the GPU: bytes equal the oracle's, both
    # verifiers accept, and the public outputs are the ones the examples print
    p, ctx = gpu
    oc = orc.circuit_of_kind(kind, param, threads=8)
    w = oc.witness(np.array(inputs, dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=17)
    gp = _prove_generic_and_compare(p, oc, w)
    got = [int(x) for x in w.public_inputs()]
    if outputs is None:
        a, b = inputs
        for _ in range(param):
            a, b = b, (a + b) % P
        outputs = [inputs[0], inputs[1], b]
    assert got == outputs, name
    # the proof carries them (ProofWithPublicInputs: u64 count + values at the end of the bytes)
    by = gp.to_bytes()
    tail = np.frombuffer(by[-8 * len(outputs):], dtype=np.uint64)
    assert [int(x) for x in tail] == outputs


@pytest.mark.parametrize("bits,value", [(6, 42), (6, 63), (1, 1), (63, 2**63 - 1), (64, 2**63 + 12345), (70, P - 1), (126, 99)])
def test_range_check_circuits_with_base_sum_gate(gpu, orc, bits, value):
    # the first gate outside the demo's five: BaseSumGate<2> (gates/base_sum.rs; 63 limbs from new_from_config), as used by
    # plonky2/examples/range_check.rs:20-24 (value = 42, log_max = 6) -> split_le (gadgets/split_join.rs:19-63): one or two gate rows,
    # unused limbs tied to zero, two rows recombined through an ArithmeticGate.  GPU proof bytes == oracle's, both verifiers accept,
    # the circuit data survives the byte form (gate tag 2 + num_limbs).  PARITY UNPINNED against a Rust proof, as every proof here.
    p, ctx = gpu
    from plonky2_demo_amd import api
    oc = orc.circuit_of_kind(7, bits, threads=8)
    w = oc.witness(np.array([value], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=bits)
    gp = _prove_generic_and_compare(p, oc, w)
    assert [int(x) for x in w.public_inputs()] == [value]
    desc = oc.product_desc()
    assert 5 in list(desc.gate_types)[:desc.num_gates]
    common = api.common_data_to_bytes(desc)
    assert common == oc.data_bytes(0)
    d2, used = api.common_data_from_bytes(common)
    assert used == len(common) and bytes(d2) == bytes(desc)
    cd = p.GenericCircuitData(desc, oc.constants_sigmas())
    vd = api.verifier_data_to_bytes(desc, cd.constants_sigmas_cap, cd.circuit_digest)
    assert api.verify_bytes(vd, gp.to_bytes()) == (True, "")
    # a proof whose range-checked value does not fit is not producible: flipping one limb opening makes both verifiers reject
    bad = bytearray(gp.to_bytes())
    bad[3 * 16 * 32 + (4 + 80) * 16 + 8 * 16] ^= 1           # an opened wire value (caps 3 x 16 x 32 B, then constants + sigmas, then wires)
    assert not cd.verify(bytes(bad))[0] and not oc.verify_bytes(bytes(bad), cd.constants_sigmas_cap, cd.circuit_digest)[0]


@pytest.mark.parametrize("kind,param", [(16, 1), (16, 2), (16, 3), (16, 4), (16, 5), (16, 6), (17, 2), (17, 5), (17, 10)])
def test_random_access_gate_circuits(gpu, orc, kind, param):
    # RandomAccessGate (gates/random_access.rs; gate_params = bits 1..6) behind CircuitBuilder::random_access, and
    # verify_merkle_proof_to_cap with a cap of four digests (hash/merkle_proofs.rs:93-150): k_quotient_random_access (a launch of its own),
    # constants hosted in the gate's extra constant wires.  GPU proof bytes == the oracle's.  PARITY UNPINNED against a Rust proof.
    from test_verifier import cap_proof_circuit_inputs
    p, ctx = gpu
    oc = orc.circuit_of_kind(kind, param, threads=8)
    if kind == 16:
        v = rand_field(param, (1 << param,))
        idx = np.array([0, (1 << param) - 1, 5 % (1 << param)], dtype=np.uint64)
        w = oc.witness(np.concatenate([v, idx]), np.zeros(0, dtype=np.uint64), filler_seed=param)
        expect = [int(i) for i in idx] + [int(v[int(i)]) for i in idx]
    else:
        index = (0x2D5 >> 1) % (1 << param)
        a, cap4 = cap_proof_circuit_inputs(orc, param, index)
        w = oc.witness(a, np.zeros(0, dtype=np.uint64), filler_seed=param)
        expect = [int(x) for x in cap4] + [index]
    _prove_generic_and_compare(p, oc, w)
    assert [int(x) for x in w.public_inputs()] == expect
    assert 9 in list(oc.product_desc().gate_types)[:oc.product_desc().num_gates]


@pytest.mark.parametrize("bits,x,y", [(9, 200, 300), (16, 255, 65535), (1, 0, 0)])
def test_a_circuit_with_every_supported_gate_type(gpu, orc, bits, x, y):
    # 11 gate types in three selector groups (oracle kind 15: two lookup tables, BaseSum<2>, Arithmetic, Exponentiation, Poseidon, ...):
    # the quotient kernels' filters across several groups, GL_MAX_GATES-sized gate arrays, 11 constant columns.  GPU bytes == oracle bytes.
    p, ctx = gpu
    oc = orc.circuit_of_kind(15, bits, threads=8)
    w = oc.witness(np.array([x, y], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=bits)
    _prove_generic_and_compare(p, oc, w)
    s = (7 * x + 1) % 256 + (3 * x * x + 5 * x + 7) % 256
    assert [int(v) for v in w.public_inputs()] == [x, y, s, pow(s + 3, y, P)]
    assert oc.product_desc().num_selectors == 3


@pytest.mark.parametrize("height,index", [(0, 0), (1, 1), (5, 13), (5, 31), (8, 170), (12, 4095)])
def test_merkle_proof_verification_circuits(gpu, orc, height, index):
    # CircuitBuilder::verify_merkle_proof (hash/merkle_proofs.rs:78-150): PoseidonGate rows with swap = 1 (the delta wires of
    # gates/poseidon.rs:113-135 are non-zero), which the demo circuit never produces: the quotient kernel's Poseidon part, the openings and
    # both verifiers on them.  GPU proof bytes == the oracle's.  PARITY UNPINNED against a Rust proof.
    from test_verifier import merkle_proof_circuit_inputs
    p, ctx = gpu
    oc = orc.circuit_of_kind(14, height, threads=8)
    a, root = merkle_proof_circuit_inputs(orc, height, index)
    w = oc.witness(a, np.zeros(0, dtype=np.uint64), filler_seed=height)
    _prove_generic_and_compare(p, oc, w)
    assert [int(x) for x in w.public_inputs()] == [int(x) for x in root] + [index]
    rows = oc.row_gates()
    wires = w.wires()
    swaps = [int(wires[24][r]) for r in range(len(rows)) if rows[r] == 4]      # PoseidonGate::WIRE_SWAP = 24
    assert sum(swaps) == bin(index).count("1")


@pytest.mark.parametrize("bits,base,exponent", [(10, 3, 1000), (64, 7, 2**63 + 5), (66, 5, P - 2), (66, P - 1, P - 1), (1, 9, 0), (7, 0, 5)])
def test_exponentiation_gate_circuits(gpu, orc, bits, base, exponent):
    # ExponentiationGate (gates/exponentiation.rs; 66 power bits, degree 4) behind CircuitBuilder::exp (gadgets/arithmetic.rs:240-272): the
    # quotient kernel's case 8 (three square-and-multiply steps at a time).  GPU proof bytes == oracle's, both verifiers accept, the public
    # output is base^exponent, a flipped intermediate-value opening is rejected by both.  PARITY UNPINNED against a Rust proof.
    p, ctx = gpu
    oc = orc.circuit_of_kind(13, bits, threads=8)
    w = oc.witness(np.array([base, exponent], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=bits)
    gp = _prove_generic_and_compare(p, oc, w)
    assert [int(x) for x in w.public_inputs()] == [base, exponent, pow(base, exponent, P)]
    desc = oc.product_desc()
    assert 8 in list(desc.gate_types)[:desc.num_gates]
    cd = p.GenericCircuitData(desc, oc.constants_sigmas())
    bad = bytearray(gp.to_bytes())
    bad[3 * 16 * 32 + (desc.num_constants + 80) * 16 + 100 * 16] ^= 1      # an opened wire value (wire 100: an intermediate value)
    assert not cd.verify(bytes(bad))[0] and not oc.verify_bytes(bytes(bad), cd.constants_sigmas_cap, cd.circuit_digest)[0]


@pytest.mark.parametrize("kind,param,inputs", [
    (8, 2, [1, 2]),                                   # lookup_test.rs test_one_lookup
    (8, 50, list(range(3, 53))),                      # two LookupGate rows, the second one padded
    (8, 40, [7] * 40),                                # one full LookupGate row, one table entry with multiplicity 40
    (8, 81, [(5 * i) % 256 for i in range(81)]),      # three LookupGate rows, n = 64 (one FRI reduction)
    (9, 3, [1000, 1037, 1333]),                       # a 10-entry table whose inputs are not their indices
    (10, 2, [3, 200, 17, 255]),                       # lookup_test.rs test_two_luts: two 256-entry tables, outputs added by an ArithmeticGate
    (10, 45, [(7 * i) % 256 for i in range(90)]),     # two tables with two LookupGate rows each
    (11, 3, [2, 9, 5, 0, 128, 255]),                  # test_different_inputs: an 8-entry table next to a 256-entry one
    (12, 2, [1, 2, 3, 4]),                            # test_same_luts: the same table added twice is stored once
])
def test_lookup_argument_circuits(gpu, orc, kind, param, inputs):
    # the lookup argument on the GPU (plonk/prover.rs:425-572: lookup polynomials; plonk/vanishing_poly.rs:503-670: their constraints in the
    # quotient; 4 extra challenges; 2 x 7 more columns in the Z batch, opened at zeta and g zeta, last in both FRI batches): proof bytes ==
    # the oracle's, both verifiers accept, outputs are the tables'.  Up to GL_MAX_LUTS tables: one LookupGate and one LookupTableGate type
    # per table, one end selector and one final-RE constraint each.  PARITY UNPINNED against a Rust proof.
    p, ctx = gpu
    oc = orc.circuit_of_kind(kind, param, threads=8)
    w = oc.witness(np.array(inputs, dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=5)
    gp = _prove_generic_and_compare(p, oc, w)
    from test_verifier import lookup_outputs
    expected, nluts = lookup_outputs(kind, param, inputs)
    assert [int(x) for x in w.public_inputs()] == expected and oc.product_desc().num_luts == nluts
    # the lookup polynomials themselves: 14 value columns behind Z and the partial products, equal to the oracle's
    zs_g, zs_o = gp.zs_partial_products(), w.prove(threads=8).zs_partial_products()
    assert zs_g.shape[0] == 34 and (zs_g == zs_o).all()
    assert zs_g[20:].any()


def test_lookup_rows_come_from_the_selector_columns(gpu, orc):
    # CommonCircuitData bytes do not hold last_lu_row (ProverOnlyCircuitData.lookup_rows, circuit_data.rs): a description read back from
    # them builds the same circuit and proves the same bytes, because build() reads the rows from the lookup selector columns; a
    # description that names a different row is refused, not proved wrongly
    p, ctx = gpu
    import copy
    from plonky2_demo_amd import api
    oc = orc.circuit_of_kind(8, 50, threads=8)
    w = oc.witness(np.arange(3, 53, dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=9)
    desc = oc.product_desc()
    d2, _ = api.common_data_from_bytes(api.common_data_to_bytes(desc))
    assert d2.last_lu_row[0] == 0 and desc.last_lu_row[0] != 0 and d2.last_lut_row[0] == desc.last_lut_row[0]
    cd = p.GenericCircuitData(d2, oc.constants_sigmas())
    assert bytes(cd.desc) == bytes(desc)              # gl_circuit_description: the rows filled in
    assert cd.prove(w.wires(), w.public_inputs()).to_bytes() == w.prove(threads=8).to_bytes()
    for field in ("last_lu_row", "last_lut_row", "first_lut_row"):
        bad = copy.copy(desc)
        getattr(bad, field)[0] += 1
        with pytest.raises(p.Plonky2Mi355xError, match="lookup"):
            p.GenericCircuitData(bad, oc.constants_sigmas())
    # two tables: the t-th LastLdc / InitSre rows and the t-th end selector are table t's
    oc2 = orc.circuit_of_kind(11, 3, threads=8)
    w2 = oc2.witness(np.array([2, 9, 5, 0, 128, 255], dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=9)
    desc2 = oc2.product_desc()
    d3, _ = api.common_data_from_bytes(api.common_data_to_bytes(desc2))
    assert [d3.last_lu_row[t] for t in range(2)] == [0, 0]
    cd2 = p.GenericCircuitData(d3, oc2.constants_sigmas())
    assert bytes(cd2.desc) == bytes(desc2)
    assert cd2.prove(w2.wires(), w2.public_inputs()).to_bytes() == w2.prove(threads=8).to_bytes()


def test_phase_api_on_a_lookup_circuit_with_an_external_transcript(gpu, orc):
    # the phase-level seam for a circuit WITH lookups: gl_partial_products_lookups / gl_quotient_polys_lookups take the delta challenges.
    # The bytes assembled by the caller equal gl_prove's and the oracle's.
    p, ctx = gpu
    oc = orc.circuit_of_kind(8, 50, threads=8)
    w = oc.witness(np.arange(3, 53, dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=9)
    wires, pis = w.wires(), w.public_inputs()
    op = w.prove(threads=8)
    cd = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas())
    r = drive_phase_api(p, ctx, orc, cd, poseidon_challenger(orc), wires, pis)
    with pytest.raises(p.Plonky2Mi355xError):
        cd.partial_products(r.d_wires.ptr, r.betas, r.gammas)              # a lookup circuit needs the deltas
    assert r.zs_b.polynomials.shape[0] == 34
    assert (r.q_b.polynomials == op.quotient_chunks()).all()
    assert r.bytes == op.to_bytes()
    assert r.bytes == cd.prove(wires, pis).to_bytes()
    assert cd.verify(r.bytes) == (True, "")


def test_prover_pool_matches_individual_proofs(gpu):
    # gl_prover_pool_*: one call, several proofs in flight on C++ threads (witness generation in HBM + prove per lane); every
    # proof equals the one produced alone on the default context, whatever lane and order it ran in
    p, ctx = gpu
    m = 20
    hc = p.MatmulCircuit(m)
    cd = hc.build()
    ops, seeds, want = [], [], []
    for k in range(11):
        a, b = rand_field(2000 + k, m * m) % (2**32 - 1), rand_field(2100 + k, m * m) % (2**32 - 1)
        ops.append((a, b)); seeds.append(50 + k)
        wires, pis = hc.witness(a, b, filler_seed=50 + k)
        want.append(cd.prove(wires, pis).to_bytes())
    pool = p.ProverPool(hc, lanes=3)
    try:
        for _ in range(2):
            got = pool.prove_matmul(ops, seeds)
            assert [g.to_bytes() for g in got] == want
        assert pool.prove_matmul([]) == []
        with pytest.raises(ValueError):
            pool.prove_matmul([(ops[0][0][:5], ops[0][1])])
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------ BASELINE config 4
def test_config4_batch_of_512_proofs_m64(gpu):
    # BASELINE.json configs[3] on one GPU: 512 independent random-witness proofs of the m = 64 circuit (operand seeds 0..511)
    # through gl_prover_pool_prove_matmul (witness generation in HBM + prove per lane); every proof accepted by gl_verify, a
    # sample of 16 byte-identical to the single-stream gl_prove of the same witness, and the Merkle caps pushed through the
    # collective the multi-GPU run uses (sharding.gather_caps; a one-rank group here, world-size 2 in tests/test_sharding.py)
    import torch.distributed as dist
    from plonky2_demo_amd import sharding
    p, ctx = gpu
    m, count = 64, 512
    hc = p.MatmulCircuit(m)

    def operands(i):
        rng = np.random.default_rng(i)
        return rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64), rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)

    ops = [operands(i) for i in range(count)]
    pool = p.ProverPool(hc, lanes=8)
    try:
        proofs = pool.prove_matmul(ops, list(range(count)))
        cap, digest = pool.constants_sigmas_cap, pool.circuit_digest
    finally:
        pool.close()
    assert len(proofs) == count and all(pr is not None for pr in proofs)
    by = [pr.to_bytes() for pr in proofs]
    assert len(set(by)) == count                                        # 512 different witnesses, 512 different proofs
    for i in range(count):
        assert hc.verify(by[i], cap, digest) == (True, ""), i
    cd = hc.build(ctx)
    assert (cd.circuit_digest == digest).all() and (cd.constants_sigmas_cap == cap).all()
    for i in range(0, count, 32):                                       # 16 of them against the single-stream prover
        a, b = ops[i]
        wires, pis = hc.witness(a, b, filler_seed=i)
        assert cd.prove(wires, pis).to_bytes() == by[i], i
    caps = np.stack([pr.caps() for pr in proofs])
    assert (caps.reshape(count, -1).view(np.uint8) == np.stack([np.frombuffer(x[:1536], dtype=np.uint8) for x in by])).all()   # the proof starts with its three caps
    own_group = not dist.is_initialized()
    if own_group:
        import socket
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        gathered = sharding.gather_caps(caps, count)
    finally:
        if own_group:
            dist.destroy_process_group()
    assert gathered.shape == (count, 3, 16, 4) and (gathered == caps).all()


# ------------------------------------------------------------------------------------------ handle / context lifetime
_LIFETIME_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import plonky2_demo_amd as p
from plonky2_demo_amd._lib import lib
ctx = p.Context(0)
rng = np.random.default_rng(1)
vals = rng.integers(0, 2**63, (5, 256), dtype=np.uint64)
batch = p.PolynomialBatch.from_values(vals, 3, False, 4, ctx=ctx)
tree = p.MerkleTree(rng.integers(0, 2**63, (64, 7), dtype=np.uint64), 2, ctx=ctx)
hc = p.MatmulCircuit(3)
cd = hc.build(ctx)
gen = hc.witness_generator(ctx)
cap_before, dig_before, cs_before = batch.cap.copy(), cd.circuit_digest.copy(), cd.constants_sigmas_cap.copy()
ctx.close()                      # the "wrong" order: the context goes first
assert (batch.cap == cap_before).all()          # handles stay usable: they keep the context alive
assert len(tree.prove(5)) == 4
assert (cd.circuit_digest == dig_before).all() and (cd.constants_sigmas_cap == cs_before).all()
del gen, cd
batch.free()
del tree                         # the last handle tears the context down
ctx2 = p.Context(0); b2 = p.PolynomialBatch.from_values(vals, 3, False, 4, ctx=ctx2)
assert (b2.cap == cap_before).all()
print("lifetime ok")             # ctx2 / b2 are finalised by the interpreter in whatever order it likes
"""


def test_handles_may_outlive_and_be_freed_after_their_context(gpu):
    # gl_ctx_destroy before gl_batch_free / gl_circuit_free / gl_merkle_free / gl_matmul_witgen_free used to be a
    # use-after-free (abort at interpreter exit); handles now hold a reference.  Run in a child so that the exit code is seen.
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LIFETIME_SCRIPT % root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "lifetime ok" in r.stdout


# ------------------------------------------------------------------------------------------ build(): sigma polynomials on the device
@pytest.mark.parametrize("m", [1, 2, 5, 20, 64])
def test_device_sigma_polynomials_equal_the_host_and_oracle_ones(gpu, orc, m):
    # gl_circuit_from_host computes the 80 sigma polynomials on the GPU from the copy-constraint classes (sigma.hip: one
    # stable radix sort instead of the reference's union-find forest, circuit_builder.rs:1007-1014); the host columns
    # (gl_host_circuit_constants_sigmas, the closed-form restatement) through gl_circuit_create must give the same
    # commitment and digest, and both must equal the oracle's (generic builder + forest)
    import ctypes
    from plonky2_demo_amd import api, _lib
    from plonky2_demo_amd._lib import check, lib
    p, ctx = gpu
    hc = p.MatmulCircuit(m)
    dev = hc.build(ctx)                                                   # sigma on the device
    host = p.GenericCircuitData(hc.desc, hc.constants_sigmas(), ctx=ctx)  # sigma columns from the host
    oc = orc.circuit(m, threads=4)
    assert (dev.circuit_digest == host.circuit_digest).all() and (dev.circuit_digest == oc.digest).all()
    assert (dev.constants_sigmas_cap == host.constants_sigmas_cap).all() and (dev.constants_sigmas_cap == oc.constants_sigmas_cap).all()
    assert (dev.constants_sigmas_batch.polynomials == host_batch_polys(p, hc, ctx)).all()
    # the class ids are only compared for equality: relabelling them (an affine bijection here) changes nothing
    cls = np.empty((80, hc.n), dtype=np.uint64)
    check(lib.gl_host_circuit_wire_classes(hc.handle, cls.ctypes.data_as(ctypes.c_void_p)))
    relabel = (cls * np.uint64(6364136223846793005) + np.uint64(1442695040888963407))      # odd multiplier: a bijection mod 2^64
    consts = np.ascontiguousarray(hc.constants_sigmas()[: hc.desc.num_constants])
    h = ctypes.c_void_p()
    check(lib.gl_circuit_create_from_classes(ctx.handle, ctypes.byref(hc.desc), consts.ctypes.data_as(ctypes.c_void_p),
                                             relabel.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)))
    try:
        dig = np.empty(4, dtype=np.uint64)
        check(lib.gl_circuit_digest(h, dig.ctypes.data_as(ctypes.c_void_p)))
        assert (dig == oc.digest).all()
    finally:
        lib.gl_circuit_free(h)


def host_batch_polys(p, hc, ctx):
    cs = hc.constants_sigmas()
    return p.PolynomialBatch.from_values(cs, 3, False, 4, ctx=ctx).polynomials
