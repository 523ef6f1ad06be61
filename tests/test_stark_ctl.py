"""GPU tests of cross-table lookups between STARK tables (csrc/stark_set.hip, csrc/stark_ctl_kernels.cuh) against the Python-integer model
tests/stark_ctl_model.py, itself pinned by tests/test_stark_ctl_model.py, on the system of tests/stark_ctl_airs.py.

degree_bits 5: 32 rows, less than a wave; 11: exactly one 2048-row segment of the scan; 12: two, so that the inclusive carry crosses a
segment boundary.
"""
import numpy as np
import pytest

import stark_ctl_airs as airs
import stark_ctl_model as cm
import stark_model as sm
from stark_model import P
from test_quotient_model import EDGES

pytestmark = pytest.mark.gpu
U64 = np.uint64
NC = 2
EDGE_CHALLENGES = [0, 1, P - 1, 2**32]
NON_CANONICAL = [P + 3, 2**64 - 1]
VARIANTS = ("random", "edges", "non-canonical")


def values_of(variant, rng, k):
    if variant == "random":
        return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]
    pool = EDGE_CHALLENGES if variant == "edges" else NON_CANONICAL
    return [pool[(i + int(rng.integers(0, len(pool)))) % len(pool)] for i in range(k)]


def challenges_of(variant, rng, nc=NC):
    flat = values_of(variant, rng, 2 * nc)
    return [(flat[2 * j], flat[2 * j + 1]) for j in range(nc)]


def flat(challenges):
    return [w for ch in challenges for w in ch]


def non_canonical(rng, trace):
    """the same field elements, a third of the words that have a second 64-bit representative by that one"""
    t = trace.copy()
    pick = (t < U64(2**32 - 1)) & (rng.integers(0, 3, size=t.shape) == 0)
    t[pick] += U64(P)
    return t


def edge_trace(rng, num_columns, n):
    """half the words edge operands, half seeded draws"""
    t = rng.integers(0, P, size=(num_columns, n), dtype=U64)
    edges = np.array(EDGES, dtype=U64)[rng.integers(0, len(EDGES), size=(num_columns, n))]
    return np.where(rng.integers(0, 2, size=(num_columns, n)) == 0, t, edges)


def set_filter(trace, table, variant):
    """the filter columns of a table: s0 and s1 of ops / ops2 (the filter is their sum), `used` of mul"""
    n = trace.shape[1]
    f = {"zero": np.zeros(n, dtype=U64), "one": np.ones(n, dtype=U64), "alternating": (np.arange(n) % 2).astype(U64)}[variant]
    if table == airs.MUL:
        trace[3] = f
    else:
        trace[3], trace[4] = f * (np.arange(n) % 3 == 0).astype(U64), f * (np.arange(n) % 3 != 0).astype(U64)


def zero_combine_row(trace, columns, challenge, i):
    """changes trace column 0 (the first Column: a single of weight 1 and power beta^0) on row i so that combine(columns(row i)) = 0"""
    assert columns[0] == ([(0, 1)], 0)
    trace[0][i] = 0
    trace[0][i] = (P - cm.combine(sm.Base, challenge, [cm.eval_table(c, trace, i) for c in columns])) % P


def model_ctl_zs(lookups, table, trace, challenges, num_tables=3):
    return [v.z for v in cm.cross_table_lookup_data([trace if t == table else None for t in range(num_tables)], lookups, challenges)[table]]


# ------------------------------------------------------------------------------- CTL Z by value
@pytest.mark.parametrize("filt", ["zero", "one", "alternating"])
@pytest.mark.parametrize("lg_n", [5, 11, 12])
def test_ctl_zs_equal_the_model_at_every_word(gpu, lg_n, filt):
    ctl_zs_equal_the_model(gpu, lg_n, filt, NC)


@pytest.mark.parametrize("nc", [3, 4])
def test_ctl_zs_of_three_and_four_challenges_equal_the_model_at_every_word(gpu, nc):
    ctl_zs_equal_the_model(gpu, 5, "alternating", nc)


def ctl_zs_equal_the_model(gpu, lg_n, filt, nc):
    p, ctx = gpu
    n = 1 << lg_n
    rng = np.random.Generator(np.random.PCG64(900 + lg_n))
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, [lg_n] * 3, airs.config(p, nc)), ctx=ctx)
    i0 = n // 2 + 3                                          # in the second segment at 2^12
    first_twc = {airs.OPS: airs.LOOKUPS[0][0][0], airs.OPS2: airs.LOOKUPS[0][0][1], airs.MUL: airs.LOOKUPS[0][1]}
    for variant in VARIANTS:
        chs = challenges_of(variant, rng, nc)
        for table, air in enumerate(airs.TABLES):
            trace = edge_trace(rng, air.num_columns, n)
            set_filter(trace, table, filt)
            twc = first_twc[table]                           # the table's first CTL Z: lookup 0 under challenge 0, zero from row i0 on
            zero_combine_row(trace, twc.columns, chs[0], i0)
            want = model_ctl_zs(airs.LOOKUPS, table, trace, chs)
            assert len(want) == sset.counts[table][1] == cm.num_ctl_zs(airs.LOOKUPS, table, nc)
            if filt == "zero":
                assert all(v == 1 for v in want[0])           # Z = 1 identically
            elif cm.eval_table(twc.filter, trace, i0) == 1:
                assert not any(want[0][i0:])
            got = sset.ctl_z_values(table, non_canonical(rng, trace), flat(chs))
            bad = np.argwhere(got != np.array(want, dtype=U64))
            assert not len(bad), "table %d, %s challenges: %d words differ, first (Z, row) %s" % (table, variant, len(bad), bad[:4].tolist())


@pytest.mark.parametrize("variant", ["edges", "non-canonical"])
@pytest.mark.parametrize("lg_n", [5, 12])
def test_ctl_zs_with_edge_and_non_canonical_coefficients(gpu, lg_n, variant):
    # every coefficient and constant of every Column drawn from the variant's pool: 0 and 1 take the product-free path, P + 3 and
    # 2^64 - 1 are reduced on upload
    p, ctx = gpu
    n = 1 << lg_n
    rng = np.random.Generator(np.random.PCG64(950 + lg_n))

    def redraw(column):
        return None if column is None else ([(c, values_of(variant, rng, 1)[0]) for c, _ in column[0]], values_of(variant, rng, 1)[0])
    lookups = [([airs.twc(t.table, [redraw(c) for c in t.columns], t.filter) for t in looking],
                airs.twc(looked.table, [redraw(c) for c in looked.columns], looked.filter)) for looking, looked in airs.LOOKUPS]
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, lookups, [lg_n] * 3, airs.config(p, NC)), ctx=ctx)
    chs = challenges_of(variant, rng)
    for table, air in enumerate(airs.TABLES):
        trace = edge_trace(rng, air.num_columns, n)
        set_filter(trace, table, "alternating")
        got = sset.ctl_z_values(table, trace, flat(chs))
        assert (got == np.array(model_ctl_zs(lookups, table, trace, chs), dtype=U64)).all()


@pytest.mark.parametrize("lg_n,row", [(5, 7), (12, 2048 + 300)])
def test_a_non_binary_filter_is_refused_not_multiplied_in(gpu, lg_n, row):
    p, ctx = gpu
    rng = np.random.Generator(np.random.PCG64(970))
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, [lg_n] * 3, airs.config(p, NC)), ctx=ctx)
    trace = edge_trace(rng, airs.ops.num_columns, 1 << lg_n)
    set_filter(trace, airs.OPS, "alternating")
    chs = flat(challenges_of("random", rng))
    sset.ctl_z_values(airs.OPS, trace, chs)                  # binary: accepted
    trace[3][row] = trace[4][row] = 1                        # s0 + s1 = 2 on one row
    with pytest.raises(p.Plonky2Mi355xError, match="non-binary CTL filter") as e:
        sset.ctl_z_values(airs.OPS, trace, chs)
    assert e.value.code == 1


@pytest.mark.parametrize("lg_n", [5, 12])
def test_the_z_batch_holds_the_permutation_zs_then_the_ctl_zs(gpu, orc, lg_n):
    # evm/src/prover.rs:332-352 for ops2 (one pair -> one permutation Z at q = 2, num_challenges = 2) and for ops (no pair)
    p, ctx = gpu
    rng = np.random.Generator(np.random.PCG64(980 + lg_n))
    lgs = [lg_n, lg_n + 1, lg_n]
    config = airs.config(p, NC)
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, config), ctx=ctx)
    traces = airs.traces(lgs, seed=lg_n)
    chs = challenges_of("random", rng)
    sets = [[tuple(values_of("random", rng, 2)) for _ in range(NC)] for _ in range(airs.ops2.q)]
    for table, perm_sets in ((airs.OPS2, sets), (airs.OPS, None)):
        air = airs.TABLES[table]
        zs_b = sset.zs(table, traces[table], None if perm_sets is None else [w for s in perm_sets for ch in s for w in ch], flat(chs))
        want = (sm.permutation_zs(air, NC, traces[table], perm_sets)[0] if perm_sets else []) + model_ctl_zs(airs.LOOKUPS, table, traces[table], chs)
        assert sset.counts[table] == (sm.num_zs(air, NC), cm.num_ctl_zs(airs.LOOKUPS, table, NC))
        assert zs_b.ncols == sum(sset.counts[table]) == len(want) and zs_b.degree == 1 << lgs[table]
        assert (orc.fft(zs_b.polynomials) == np.array(want, dtype=U64)).all()
        ref = p.PolynomialBatch.from_values(list(np.array(want, dtype=U64)), config.rate_bits, False, config.cap_height, ctx=ctx)
        assert (zs_b.cap == ref.cap).all()
    with pytest.raises(p.Plonky2Mi355xError, match="permutation challenge sets go with permutation pairs"):
        sset.zs(airs.OPS2, traces[airs.OPS2], None, flat(chs))


def test_consistent_traces_multiply_out_across_tables(gpu):
    # Z[n - 1] is what the verifier multiplies across tables (cross_table_lookup.rs:542-569): with device-made Zs of a consistent system
    # the looking products equal the looked value, and with one looked row removed they do not
    p, ctx = gpu
    lgs = [5, 6, 5]
    rng = np.random.Generator(np.random.PCG64(990))
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, airs.config(p, NC)), ctx=ctx)
    chs = challenges_of("random", rng)
    good = airs.traces(lgs, seed=1)
    for traces, consistent in ((good, True), (airs.remove_one_looked_row(good), False)):
        assert cm.check_ctls(traces, airs.LOOKUPS) == consistent
        lasts = [[int(v) for v in sset.ctl_z_values(t, traces[t], flat(chs))[:, -1]] for t in range(3)]
        assert cm.verify_cross_table_lookups(airs.LOOKUPS, lasts, NC) == consistent


# ------------------------------------------------------------------------------- quotient by value at every coset point
def through_points(orc, targets, lg_n, rate_bits, k):
    """the value columns (on H_n) of the polynomials of degree < n that take `targets` on the LDE points i = k (mod 2^rate_bits)"""
    from vanishing_model import primitive_root
    shift = 7 * pow(primitive_root(lg_n + rate_bits), k, P) % P
    return orc.fft(orc.coset_ifft(targets, shift))


def permutation_sets(variant, rng, air, nc):
    return [[tuple(values_of(variant, rng, 2)) for _ in range(nc)] for _ in range(air.q)] if air.pairs else None


def flat_sets(sets):
    return None if sets is None else [w for s in sets for ch in s for w in ch]


# the CTL checks alone (ops, mul) and after a permutation pair's (ops2); 2^12 crosses many blocks and the wrap-around of `next`
@pytest.mark.parametrize("table,lg_n,nc,variants", [(airs.OPS, 5, 2, VARIANTS), (airs.OPS2, 5, 2, VARIANTS), (airs.MUL, 5, 1, VARIANTS),
                                                    (airs.OPS2, 5, 1, VARIANTS), (airs.OPS2, 12, 2, ("edges",)), (airs.MUL, 12, 1, ("non-canonical",)),
                                                    (airs.OPS2, 5, 3, VARIANTS), (airs.MUL, 5, 3, VARIANTS), (airs.OPS2, 5, 4, VARIANTS), (airs.MUL, 5, 4, VARIANTS)])
def test_quotient_values_equal_the_model_at_every_coset_point(gpu, orc, table, lg_n, nc, variants):
    quotient_values_equal_the_model(gpu, orc, airs.TABLES, table, lg_n, nc, variants)


@pytest.mark.parametrize("table,nc", [(airs.MUL, 2), (airs.MUL, 3), (airs.OPS2, 4)])
def test_quotient_values_beside_a_degree_5_table_equal_the_model_at_every_coset_point(gpu, orc, table, nc):
    # mul at q = 4: four values of 1 / Z_H, alpha^(2 nctl) after a longer single-table part; ops2 at q = 2 on every second LDE point
    assert [(a.q, 1 << (a.rate_bits - a.qdb)) for a in airs.TABLES5] == [(2, 2), (2, 2), (4, 1)]
    quotient_values_equal_the_model(gpu, orc, airs.TABLES5, table, 5, nc, VARIANTS)


def quotient_values_equal_the_model(gpu, orc, tables, table, lg_n, nc, variants):
    from test_quotient_model import edge_targets
    p, ctx = gpu
    air = tables[table]
    n, size = 1 << lg_n, (1 << lg_n) << air.qdb
    step = 1 << (air.rate_bits - air.qdb)
    rng = np.random.Generator(np.random.PCG64(1100 + 10 * lg_n + table))
    config = airs.config(p, nc, air.rate_bits)
    sset = p.StarkSet(airs.api_set(p, tables, airs.LOOKUPS, [lg_n] * 3, config), ctx=ctx)
    nzs = sum(sset.counts[table])
    k = step * int(rng.integers(0, 1 << air.qdb))                    # a multiple of step: the quotient coset sees the edge rows
    edge_points = np.arange(k, n << air.rate_bits, 1 << air.rate_bits)
    t_trace = edge_targets(rng, air.num_columns, n)
    trace_b = p.PolynomialBatch.from_values(list(through_points(orc, t_trace, lg_n, air.rate_bits, k)), air.rate_bits, False, config.cap_height, ctx=ctx)
    zs_b = p.PolynomialBatch.from_values(list(through_points(orc, edge_targets(rng, nzs, n), lg_n, air.rate_bits, k)), air.rate_bits, False, config.cap_height, ctx=ctx)
    trace_lde, zs_lde = trace_b.lde_values(), zs_b.lde_values()
    assert (trace_lde[:, edge_points] == t_trace).all()
    for variant in variants:
        sets, chs, alphas = permutation_sets(variant, rng, air, nc), challenges_of(variant, rng, nc), values_of(variant, rng, nc)
        got = sset.quotient_values(table, trace_b, zs_b, flat_sets(sets), flat(chs), alphas, [])
        assert got.shape == (nc, size)
        ctl_data = cm.cross_table_lookup_data([None] * 3, airs.LOOKUPS, chs)[table]
        want = np.array(cm.quotient_values(orc, air, nc, lg_n, trace_lde[:, ::step], zs_lde[:, ::step], sets, alphas, [], ctl_data), dtype=U64)
        bad = np.argwhere(got != want)
        assert not len(bad), "table %d at 2^%d, %s variant: %d of %d words differ, first (challenge, point) %s" % (table, lg_n, variant, len(bad), nc * size, bad[:4].tolist())
    if table == airs.OPS2:                                           # the CTL pass changes the words k_stark_quotient alone leaves
        alone = p.Stark(sset.desc.tables[table][0], config, lg_n, ctx=ctx)
        perm_b = p.PolynomialBatch.from_values(list(orc.fft(zs_b.polynomials)[:sset.counts[table][0]]), air.rate_bits, False, config.cap_height, ctx=ctx)
        assert (alone.quotient_values(trace_b, perm_b, flat_sets(sets), alphas, []) != got).any()


@pytest.mark.parametrize("nc", [1, 2])
def test_quotient_polys_of_a_consistent_system_are_the_model_s_chunks(gpu, orc, nc):
    # the phase entries in the prover's order on real Zs: gl_stark_set_zs, then gl_stark_set_quotient_polys; the chunks are the model's
    p, ctx = gpu
    lgs = [5, 6, 5]
    rng = np.random.Generator(np.random.PCG64(1200 + nc))
    config = airs.config(p, nc)
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, config), ctx=ctx)
    traces = airs.traces(lgs, seed=4)
    chs = challenges_of("random", rng, nc)
    data = cm.cross_table_lookup_data(traces, airs.LOOKUPS, chs)
    for table, air in enumerate(airs.TABLES):
        n = 1 << lgs[table]
        sets, alphas = permutation_sets("random", rng, air, nc), values_of("random", rng, nc)
        trace_b = p.PolynomialBatch.from_values(list(traces[table]), air.rate_bits, False, config.cap_height, ctx=ctx)
        zs_b = sset.zs(table, traces[table], flat_sets(sets), flat(chs))
        q_b = sset.quotient_polys(table, trace_b, zs_b, flat_sets(sets), flat(chs), alphas, [])
        assert q_b.ncols == nc * air.q and q_b.degree == n
        step = 1 << (air.rate_bits - air.qdb)
        values = cm.quotient_values(orc, air, nc, lgs[table], trace_b.lde_values()[:, ::step], zs_b.lde_values()[:, ::step], sets, alphas, [], data[table])
        want = orc.coset_ifft(np.array(values, dtype=U64), 7)[:, :air.q * n].reshape(nc * air.q, n)
        assert (q_b.polynomials == want).all()
        with pytest.raises(p.Plonky2Mi355xError, match="Z batch does not match"):
            sset.quotient_polys(table, trace_b, trace_b, flat_sets(sets), flat(chs), alphas, [])


# ------------------------------------------------------------------------------- whole set proofs
def model_challenger(orc, hasher):
    from test_fri_openings import model_challenger as base
    b = base(orc, hasher)
    return cm.CompactChallenger(b.permute, b.hash_elements)


def cap_builder(orc, hasher, rate_bits, cap_height):
    """Merkle caps rebuilt by the model's Merkle code: the oracle's under Poseidon, test_keccak.ModelTree over the oracle's LDE under Keccak"""
    if hasher == "poseidon":
        return lambda cols, values: orc.batch(cols, rate_bits, cap_height, from_values=values).cap.tolist()
    import test_keccak

    def cap(cols, values):
        lde = orc.lde(orc.ifft(cols) if values else np.asarray(cols, dtype=U64), rate_bits)
        lgN = lde.shape[1].bit_length() - 1
        order = [int(format(i, "0%db" % lgN)[::-1], 2) for i in range(1 << lgN)]
        return test_keccak.ModelTree(lde.T[order]).cap(cap_height).tolist()
    return cap


def check_set_proof(p, orc, tables, lookups, lgs, nc, hasher, sset, proof, traces, max_queries=None, quotient=True):
    """caps rebuilt, openings (ctl_zs_last among them) recomputed, the transcript replayed by the model verifier, both verifiers accept"""
    from prover_phase_model import eval_ext
    from test_fri_openings import verify_path_of
    from vanishing_model import primitive_root
    config = sset.desc.config
    params = [sset.desc.fri_params(t) for t in range(len(tables))]
    assert len(proof) == sset.proof_size == sum(cm.table_proof_size(a, nc, cm.num_ctl_zs(lookups, t, nc), params[t]) for t, a in enumerate(tables))
    seen = {}
    assert cm.verify_set(tables, lookups, nc, params, proof, model_challenger(orc, hasher), verify_path_of(orc, hasher), max_queries=max_queries, trace=seen) == (0, len(tables))
    assert sset.verify(proof) == (True, "", 0, len(tables))
    cap = cap_builder(orc, hasher, config.rate_bits, config.cap_height)
    data = cm.cross_table_lookup_data(traces, lookups, seen["ctl_challenges"])
    for t, (air, sub) in enumerate(zip(tables, seen["tables"])):
        pp, zeta, g = sub["table_proof"], sub["zeta"], primitive_root(lgs[t])
        zs = (sm.permutation_zs(air, nc, traces[t], sub["sets"])[0] if air.pairs else []) + [v.z for v in data[t]]
        assert pp.trace_cap == cap(traces[t], True) and pp.zs_cap == cap(np.array(zs, dtype=U64), True)
        assert pp.ctl_zs_last == [v.z[-1] for v in data[t]]              # Z(g^-1) is the last row's value
        gzeta = (zeta[0] * g % P, zeta[1] * g % P)
        trace_coeffs, zs_coeffs = orc.ifft(traces[t]), orc.ifft(np.array(zs, dtype=U64))
        assert pp.local == [eval_ext(c, zeta) for c in trace_coeffs] and pp.next == [eval_ext(c, gzeta) for c in trace_coeffs]
        assert pp.zs == [eval_ext(c, zeta) for c in zs_coeffs] and pp.zs_next == [eval_ext(c, gzeta) for c in zs_coeffs]
        if quotient:
            step = 1 << (air.rate_bits - air.qdb)
            values = cm.quotient_values(orc, air, nc, lgs[t], orc.lde(trace_coeffs, air.rate_bits)[:, ::step], orc.lde(zs_coeffs, air.rate_bits)[:, ::step],
                                        sub["sets"], sub["alphas"], [], data[t])
            chunks = orc.coset_ifft(np.array(values, dtype=U64), 7)[:, :air.q << lgs[t]].reshape(nc * air.q, 1 << lgs[t])
            assert pp.quotient_cap == cap(chunks, False) and pp.quotient == [eval_ext(c, zeta) for c in chunks]


@pytest.mark.parametrize("lgs,nc,hasher", [([5, 6, 5], 2, "poseidon"), ([5, 6, 5], 1, "poseidon"), ([5, 6, 5], 2, "keccak"), ([12, 11, 12], 2, "poseidon"),
                                           ([5, 6, 5], 4, "poseidon")])
def test_whole_set_proof(gpu, orc, lgs, nc, hasher):
    p, ctx = gpu
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, airs.config(p, nc), hasher=hasher), ctx=ctx)
    traces = airs.traces(lgs, seed=7)
    proof = sset.prove(traces)
    small = lgs[0] == 5
    check_set_proof(p, orc, airs.TABLES, airs.LOOKUPS, lgs, nc, hasher, sset, proof, traces, max_queries=None if small else 4, quotient=small)
    if small:
        assert sset.prove(traces) == proof, "two calls on the same input give different bytes"
        rng = np.random.Generator(np.random.PCG64(77))
        other = [t.copy() for t in traces]
        for t in other:                                          # every word that has a second representative, by that one
            t[t < U64(2**32 - 1)] += U64(P)
        assert any((a != b).any() for a, b in zip(other, traces)) and sset.prove(other) == proof, "non-canonical traces give other bytes"
        del rng


def test_an_inconsistent_system_is_rejected_by_the_cross_table_check(gpu, orc):
    # one looked row removed: every table still satisfies its own AIR and its own CTL checks, so every table's proof verifies; only the
    # product across tables fails, last of all
    from test_fri_openings import verify_path_of
    p, ctx = gpu
    lgs, nc = [5, 6, 5], 2
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, airs.config(p, nc)), ctx=ctx)
    traces = airs.remove_one_looked_row(airs.traces(lgs, seed=8))
    proof = sset.prove(traces)
    ok, why, code, table = sset.verify(proof)
    assert (ok, code, table) == (False, p._lib.GL_CHECK_CTL, 3) and "ross-table" in why
    params = [sset.desc.fri_params(t) for t in range(3)]
    assert cm.verify_set(airs.TABLES, airs.LOOKUPS, nc, params, proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == (cm.CTL, 3)


def test_whole_set_proof_with_a_degree_5_table_and_its_inconsistent_system(gpu, orc):
    # tables of q = 2 and q = 4 in one set under rate_bits 2
    from test_fri_openings import verify_path_of
    p, ctx = gpu
    lgs, nc = [5, 6, 5], 3
    sset = p.StarkSet(airs.api_set(p, airs.TABLES5, airs.LOOKUPS, lgs, airs.config(p, nc, airs.RATE_BITS5)), ctx=ctx)
    assert [sset.desc.fri_params(t).rate_bits for t in range(3)] == [2, 2, 2]
    traces = airs.traces(lgs, seed=7)
    proof = sset.prove(traces)
    check_set_proof(p, orc, airs.TABLES5, airs.LOOKUPS, lgs, nc, "poseidon", sset, proof, traces)
    removed = sset.prove(airs.remove_one_looked_row(traces))
    ok, why, code, table = sset.verify(removed)
    assert (ok, code, table) == (False, p._lib.GL_CHECK_CTL, 3) and "ross-table" in why
    params = [sset.desc.fri_params(t) for t in range(3)]
    assert cm.verify_set(airs.TABLES5, airs.LOOKUPS, nc, params, removed, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == (cm.CTL, 3)


def test_a_single_table_set_with_one_permutation_pair(gpu, orc):
    # no CTL at all: the set path (compact, the Z cap always present, a two-batch instance) does not depend on having one
    import stark_airs
    p, ctx = gpu
    air, lg_n, nc = stark_airs.cubic, 5, 2
    trace, pis = air.trace(1 << lg_n, seed=3)
    config = airs.config(p, nc)
    sset = p.StarkSet(airs.api_set(p, [air], [], [lg_n], config), ctx=ctx)
    assert sset.counts == [(1, 0)]
    proof = sset.prove([trace], [pis])
    from test_fri_openings import verify_path_of
    assert sset.verify(proof) == (True, "", 0, 1)
    assert cm.verify_set([air], [], nc, [sset.desc.fri_params(0)], proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == (0, 1)
    flipped = bytearray(proof)
    flipped[-8] ^= 1                                             # the public input x0: the first-row constraint no longer holds at zeta
    assert sset.verify(bytes(flipped))[2:] == (sm.VANISHING, 0)


def test_the_phase_entries_driven_from_python_reproduce_the_one_call_bytes(gpu, orc):
    # prove_with_traces on the Python Challenger (compact per table) and the phase entries: byte for byte gl_stark_set_prove's proof
    from vanishing_model import primitive_root
    p, ctx = gpu
    lgs, nc = [5, 6, 5], 2
    config = airs.config(p, nc)
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, config), ctx=ctx)
    traces = airs.traces(lgs, seed=9)
    ch = p.Challenger()
    trace_bs = [p.PolynomialBatch.from_values(list(t), config.rate_bits, False, config.cap_height, ctx=ctx) for t in traces]
    for b in trace_bs:
        ch.observe_hashes(b.cap)
    ctl = ch.get_n_challenges(2 * nc)
    out = b""
    words = lambda a: np.asarray(a, dtype="<u8").tobytes()      # noqa: E731
    for t, air in enumerate(airs.TABLES):
        params = sset.desc.fri_params(t)
        nz, nctl = sset.counts[t]
        ch.compact()
        sets = ch.get_n_challenges(2 * air.q * nc) if nz else None
        zs_b = sset.zs(t, traces[t], sets, ctl)
        ch.observe_hashes(zs_b.cap)
        alphas = ch.get_n_challenges(nc)
        q_b = sset.quotient_polys(t, trace_bs[t], zs_b, sets, ctl, alphas, [])
        ch.observe_hashes(q_b.cap)
        zeta = ch.get_n_challenges(2)
        g = primitive_root(lgs[t])
        gzeta, last = [zeta[0] * g % P, zeta[1] * g % P], [pow(g, P - 2, P), 0]
        local, nxt, zl, zn, ql = trace_bs[t].open_at(zeta), trace_bs[t].open_at(gzeta), zs_b.open_at(zeta), zs_b.open_at(gzeta), q_b.open_at(zeta)
        lasts = zs_b.open_at(last, nz, nctl)
        assert not np.asarray(lasts).reshape(-1, 2)[:, 1].any()
        for v in (local, zl, ql, nxt, zn, lasts):
            ch.observe_elements(v)
        inst = cm.fri_instance(air, nc, nctl, zeta, lgs[t])
        fri = p.PolynomialBatch.prove_openings(p.FriInstance(inst.oracles, inst.batches), [trace_bs[t], zs_b, q_b], ch, params, ctx=ctx)
        out += words(trace_bs[t].cap) + words(zs_b.cap) + words(q_b.cap) + words(local) + words(nxt) + words(zl) + words(zn)
        out += words(np.asarray(lasts).reshape(-1, 2)[:, 0]) + words(ql) + bytes(fri)
    assert out == sset.prove(traces)


def quartic_set(p, ctx, lg_n, nc):
    """stark_airs.quartic (degree 4, rate_bits 2: q = 3, a quotient coset of 4 n points, so trim_to_len(3 n) has a tail) looking its own
    column 2 up in its column 3, which its trace generator makes a permutation of column 2: one table, looking and looked"""
    import stark_airs
    air = stark_airs.quartic
    lookups = [([airs.twc(0, [airs.single(2)])], airs.twc(0, [airs.single(3)]))]
    config = p.StarkConfig.standard_fast_config()
    config.num_challenges, config.rate_bits = nc, air.rate_bits
    return air, lookups, p.StarkSet(airs.api_set(p, [air], lookups, [lg_n], config), ctx=ctx), config


def test_a_ctl_z_computed_under_other_challenges_is_refused(gpu):
    p, ctx = gpu
    lg_n, nc = 5, 2
    air, lookups, sset, config = quartic_set(p, ctx, lg_n, nc)
    rng = np.random.Generator(np.random.PCG64(1300))
    trace, pis = air.trace(1 << lg_n, seed=2)
    assert cm.check_ctls([trace], lookups)
    sets, chs, alphas = permutation_sets("random", rng, air, nc), challenges_of("random", rng, nc), values_of("random", rng, nc)
    trace_b = p.PolynomialBatch.from_values(list(trace), config.rate_bits, False, config.cap_height, ctx=ctx)
    zs_b = sset.zs(0, trace, flat_sets(sets), flat(chs))
    assert sset.quotient_polys(0, trace_b, zs_b, flat_sets(sets), flat(chs), alphas, pis).ncols == nc * air.q
    other = [(chs[0][0], (chs[0][1] + 1) % P)] + chs[1:]            # one gamma changed
    with pytest.raises(p.Plonky2Mi355xError, match="does not satisfy the constraints") as e:
        sset.quotient_polys(0, trace_b, zs_b, flat_sets(sets), flat(other), alphas, pis)
    assert e.value.code == 1


def test_whole_set_proof_at_q_3_with_a_table_looking_into_itself(gpu, orc):
    p, ctx = gpu
    lg_n, nc = 5, 2
    air, lookups, sset, config = quartic_set(p, ctx, lg_n, nc)
    trace, pis = air.trace(1 << lg_n, seed=2)
    proof = sset.prove([trace], [pis])
    from test_fri_openings import verify_path_of
    assert sset.verify(proof) == (True, "", 0, 1)
    assert cm.verify_set([air], lookups, nc, [sset.desc.fri_params(0)], proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == (0, 1)


def test_the_committed_fixture_is_current(gpu):
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import make_stark_ctl_fixture as tool
    proof, meta = tool.make()
    with open(os.path.join(root, "tests", "golden", "stark_ctl_set.bin"), "rb") as f:
        assert f.read() == proof, "tests/golden/stark_ctl_set.bin is stale: run tools/make_stark_ctl_fixture.py on the GPU"
    with open(os.path.join(root, "tests", "golden", "stark_ctl_set.json")) as f:
        assert json.load(f) == meta
