"""CPU tests that pin tests/stark_model.py, the Python-integer model the GPU tests of the STARK kernels compare against: on satisfying
traces of every AIR of tests/stark_airs.py, under every num_challenges gl_stark_check admits, the quotient passes the reference's degree check -- which is also what confirms the
factor bound gl_stark_check enforces -- the identity C(zeta) = Z_H(zeta) t(zeta) holds at an extension point,
and one changed trace cell breaks it."""
import numpy as np
import pytest

import stark_airs
import stark_model as sm
from stark_model import P
from vanishing_model import primitive_root

LG_N = 5
NCS = (1, 2, 3, 4)                                # every num_challenges gl_stark_check admits
U64 = np.uint64


# every AIR under every count; the standard configuration's two keep the plain name
AIRS_X_NCS = [pytest.param(name, nc, id=name if nc == 2 else "%s-nc%d" % (name, nc)) for name in stark_airs.AIRS for nc in NCS]


def draw(rng, k):
    return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]


def challenge_sets(rng, air, nc):
    return [[tuple(draw(rng, 2)) for _ in range(nc)] for _ in range(air.q)]


def quotient_of(orc, air, nc, trace, pis, sets, alphas):
    """the model prover's path: Z polynomials, LDEs onto the quotient coset, quotient values, chunks (None: the degree check failed)"""
    zs = sm.permutation_zs(air, nc, trace, sets)[0] if air.pairs else []
    trace_coeffs = orc.ifft(trace)
    zs_coeffs = orc.ifft(np.array(zs, dtype=U64)) if zs else np.zeros((0, 1 << LG_N), dtype=U64)
    trace_q = orc.lde(trace_coeffs, air.qdb)
    zs_q = orc.lde(zs_coeffs, air.qdb) if zs else []
    values = sm.quotient_values(orc, air, nc, LG_N, trace_q, zs_q, sets, alphas, pis)
    return trace_coeffs, zs_coeffs, sm.quotient_chunks(orc, air, nc, LG_N, values)


def identity_at(air, nc, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas):
    from prover_phase_model import eval_ext
    g = primitive_root(LG_N)
    gzeta = (zeta[0] * g % P, zeta[1] * g % P)
    local, nxt = [eval_ext(c, zeta) for c in trace_coeffs], [eval_ext(c, gzeta) for c in trace_coeffs]
    zl, zn = [eval_ext(c, zeta) for c in zs_coeffs], [eval_ext(c, gzeta) for c in zs_coeffs]
    vanishing = sm.vanishing_at(air, nc, LG_N, zeta, local, nxt, pis, alphas, zl, zn, sets)
    return sm.identity_holds(air, nc, LG_N, zeta, vanishing, [eval_ext(c, zeta) for c in chunks])


@pytest.mark.parametrize("name,nc", AIRS_X_NCS)
def test_satisfying_trace_passes_the_degree_check_and_the_identity(orc, name, nc):
    air = stark_airs.AIRS[name]
    rng = np.random.Generator(np.random.PCG64(11))
    trace, pis = air.trace(1 << LG_N, seed=1)
    sets, alphas, zeta = challenge_sets(rng, air, nc), draw(rng, nc), tuple(draw(rng, 2))
    trace_coeffs, zs_coeffs, chunks = quotient_of(orc, air, nc, trace, pis, sets, alphas)
    # quotient degree < q n with terms of up to q + 1 trace factors (q under a row filter): the bound gl_stark_check enforces is enough
    longest = max(sum(1 for kind, _ in ops if kind != stark_airs.PUBLIC) for _, terms in air.constraints for _, ops in terms)
    assert longest == air.longest and LONGEST[name] == longest
    assert chunks is not None, "the quotient of a satisfying trace fails trim_to_len(q n)"
    assert chunks.shape == (nc * air.q, 1 << LG_N)
    assert identity_at(air, nc, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas)


# the largest number of trace factors in a term: q + 1, the bound itself, except where the recurrence is linear in the trace
LONGEST = {"fibonacci": 1, "cubic": 3, "quartic": 4, "wide": 2, "quintic": 5, "sextic": 6, "nonic": 9, "linear": 1, "pairs33": 2, "longpair": 3,
           "manyfactors": 2, "nopublic": 2}
WIDE = {"wide": 6, "longpair": 5, "pairs33": 5}          # 67 to 130 columns or 33 pairs: each evaluation is long, so fewer cells


@pytest.mark.parametrize("name,nc", AIRS_X_NCS)
def test_one_changed_cell_breaks_the_identity(orc, name, nc):
    air = stark_airs.AIRS[name]
    n = 1 << LG_N
    rng = np.random.Generator(np.random.PCG64(12))
    trace, pis = air.trace(n, seed=2)
    sets, alphas, zeta = challenge_sets(rng, air, nc), draw(rng, nc), tuple(draw(rng, 2))
    perm_columns = sorted({c for pair in air.pairs for lr in pair for c in lr})
    cells = [(0, 0), (0, n - 1), (air.num_columns - 1, 0), (air.num_columns - 1, n - 1)] + [(c, r) for c in perm_columns[:4] for r in (0, n - 1)]
    cells += [(int(rng.integers(0, air.num_columns)), int(rng.integers(0, n))) for _ in range(4)]
    if name in WIDE:
        cells = cells[:4] + cells[-(WIDE[name] - 4):]    # the four corners and random cells
    for col, row in cells:
        bad = trace.copy()
        bad[col, row] = (int(bad[col, row]) + 1) % P
        zs = sm.permutation_zs(air, nc, bad, sets)[0] if air.pairs else []
        trace_coeffs = orc.ifft(bad)
        zs_coeffs = orc.ifft(np.array(zs, dtype=U64)) if zs else np.zeros((0, n), dtype=U64)
        values = sm.quotient_values(orc, air, nc, LG_N, orc.lde(trace_coeffs, air.qdb), orc.lde(zs_coeffs, air.qdb) if zs else [], sets, alphas, pis)
        # without the trim the "quotient" is the interpolant of C / Z_H on the coset: its first q n coefficients stand in for the chunks
        coeffs = orc.coset_ifft(np.array(values, dtype=U64), 7)
        chunks = coeffs[:, :air.q * n].reshape(nc * air.q, n)
        assert not identity_at(air, nc, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas), \
            "changing cell (column %d, row %d) of %s goes unnoticed" % (col, row, name)


def test_fibonacci_constraints_equal_a_hand_written_evaluation():
    # the five constraints of fibonacci_stark.rs:72-85 written out, not through the term list
    air = stark_airs.fibonacci
    rng = np.random.Generator(np.random.PCG64(13))
    for it in range(8):
        local, nxt, pub = draw(rng, 4), draw(rng, 4), draw(rng, 3)
        want = [(local[0] - pub[0]) % P, (local[1] - pub[1]) % P, (local[1] - pub[2]) % P, (nxt[0] - local[1]) % P, (nxt[1] - local[0] - local[1]) % P]
        assert sm.constraint_values(sm.Base, air, local, nxt, pub) == want
        nc = NCS[it % len(NCS)]                          # the consumer under every number of alphas
        alphas, z_last, lf, ll = draw(rng, nc), draw(rng, 1)[0], draw(rng, 1)[0], draw(rng, 1)[0]
        filters = [lf, lf, ll, z_last, z_last]
        accs = [0] * nc
        for c, f in zip(want, filters):
            accs = [(a * al + c * f) % P for a, al in zip(accs, alphas)]
        assert sm.eval_vanishing(sm.Base, stark_airs._air("f", 4, 3, 2, 1, air.constraints, [], None), nc, local, nxt, pub, alphas, z_last, lf, ll) == accs
    assert [f for f, _ in air.constraints] == [stark_airs.FIRST_ROW] * 2 + [stark_airs.LAST_ROW] + [stark_airs.TRANSITION] * 2


@pytest.mark.parametrize("name,nc,nz", [pytest.param(name, nc, nz, id=name if nc == 2 and name != "pairs33" else "%s-nc%d" % (name, nc)) for name, nc, nz in [
    ("fibonacci", 2, 2), ("cubic", 2, 1), ("quartic", 2, 2), ("quintic", 3, 3), ("sextic", 4, 2), ("nonic", 3, 2), ("nonic", 1, 1), ("linear", 1, 1),
    ("pairs33", 2, 66), ("pairs33", 1, 33), ("pairs33", 4, 132), ("longpair", 3, 2)]])
def test_z_starts_at_one_and_the_quotients_multiply_to_one(name, nc, nz):
    air = stark_airs.AIRS[name]
    rng = np.random.Generator(np.random.PCG64(14))
    trace, _ = air.trace(1 << LG_N, seed=3)
    zs, quotients = sm.permutation_zs(air, nc, trace, challenge_sets(rng, air, nc))
    assert len(zs) == sm.num_zs(air, nc) == nz
    for z, quot in zip(zs, quotients):
        total = 1
        for v in quot:
            total = total * v % P
        assert z[0] == 1 and total == 1 and z[-1] * quot[-1] % P == 1


def test_batches_take_the_challenges_the_reference_takes():
    # get_permutation_batches (permutation.rs:228-249): the set index is the position INSIDE the chunk
    assert sm.permutation_batches(stark_airs.cubic, 2) == [[(0, 0, 0), (0, 1, 1)]]
    assert sm.permutation_batches(stark_airs.quartic, 2) == [[(0, 0, 0), (0, 1, 1), (1, 2, 0)], [(1, 0, 1), (2, 1, 0), (2, 2, 1)]]
    assert sm.permutation_batches(stark_airs.fibonacci, 2) == [[(0, 0, 0)], [(0, 0, 1)]]
    # one pair, three challenges, q = 2: the last batch holds ONE instance, which takes set 0
    assert sm.permutation_batches(stark_airs.longpair, 3) == [[(0, 0, 0), (0, 1, 1)], [(0, 0, 2)]]
    # q = 1: a batch per instance, all on set 0; 66 of them, pair after pair
    batches = sm.permutation_batches(stark_airs.pairs33, 2)
    assert len(batches) == 66 and batches[0] == [(0, 0, 0)] and batches[1] == [(0, 0, 1)] and batches[64] == [(32, 0, 0)] and batches[65] == [(32, 0, 1)]
    # q = 8 over 3 pairs x 4 challenges: a full batch, then a partial one of four
    assert sm.permutation_batches(stark_airs.nonic, 4) == [[(0, 0, 0), (0, 1, 1), (0, 2, 2), (0, 3, 3), (1, 4, 0), (1, 5, 1), (1, 6, 2), (1, 7, 3)],
                                                          [(2, 0, 0), (2, 1, 1), (2, 2, 2), (2, 3, 3)]]


def test_the_airs_cover_every_shape_the_gpu_tests_are_meant_to_run():
    # the matrix guard: the GPU tests take their shapes from AIRS x num_challenges; removing an AIR must fail here, not narrow them silently
    ncs, qs, qdbs, steps = set(), set(), set(), set()
    strided_coset = many_zs = partial_batch = pair_of_64 = term_of_64 = no_public = False
    for air in stark_airs.AIRS.values():
        pair_of_64 |= any(len(pair) == 64 for pair in air.pairs)
        term_of_64 |= any(len(ops) == 64 for _, terms in air.constraints for _, ops in terms)
        no_public |= air.num_public_inputs == 0
        for nc in NCS:
            step, nz, instances = 1 << (air.rate_bits - air.qdb), sm.num_zs(air, nc), len(air.pairs) * nc
            ncs.add(nc), qs.add(air.q), qdbs.add(air.qdb), steps.add(step)
            strided_coset |= step > 1 and air.qdb > 0
            many_zs |= nz > 64
            partial_batch |= instances % air.q != 0 and nz > 1
    assert ncs == {1, 2, 3, 4} and qs >= {1, 2, 3, 4, 5, 8} and qdbs == {0, 1, 2, 3} and steps >= {1, 2}
    assert strided_coset and many_zs and partial_batch and pair_of_64 and term_of_64 and no_public


def test_the_edge_traces_of_the_gpu_z_cases_are_free_of_zero_denominators():
    # tests/test_stark.py arranges a trace of edge operands per case, at most 64 rounds of drawing again: that it gets there needs no GPU.
    # (The 4096-row cases are left to the GPU test itself, which asserts the same.)
    import test_stark
    cases = [c.values for c in test_stark.Z_CASES if c.values[1] <= 8]
    assert {(name, nc) for name, _, nc in cases} >= {("pairs33", 2), ("pairs33", 4), ("longpair", 3), ("nonic", 3), ("linear", 1)}
    for name, lg_n, nc in cases:
        air = stark_airs.AIRS[name]
        all_sets, trace = test_stark.edge_trace_for_the_zs(air, nc, lg_n)
        assert set(all_sets) == set(test_stark.VARIANTS) and trace.shape == (air.num_columns, 1 << lg_n)
        for sets in all_sets.values():
            assert all(all(den) for _, den in sm.permutation_num_den(air, nc, trace, sets))
        # the edge pool's gammas are all minus an edge operand: on single-column pairs a cell had to be moved out of the way
        assert all((P - g) % P in test_stark.EDGES for s in all_sets["edges"] for _, g in s)


def test_lagrange_selectors_on_the_coset_equal_the_closed_forms(orc):
    # L_first(x) = Z_H(x) / (n (x - 1)), L_last(x) = Z_H(x) g^-1 / (n (x - g^-1)): what the kernels use, against the LDE of the selectors
    for qdb in (0, 1, 2, 3):
        lf, ll = sm.lagrange_on_coset(orc, LG_N, qdb)
        n, w, last = 1 << LG_N, primitive_root(LG_N + qdb), pow(primitive_root(LG_N), P - 2, P)
        for i in range(n << qdb):
            x = 7 * pow(w, i, P) % P
            zh = (pow(x, n, P) - 1) % P
            assert lf[i] == zh * pow(n * (x - 1) % P, P - 2, P) % P
            assert ll[i] == zh * last % P * pow(n * (x - last) % P, P - 2, P) % P
