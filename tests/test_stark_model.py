"""CPU tests that pin tests/stark_model.py, the Python-integer model the GPU tests of the STARK kernels compare against: on satisfying
traces of the four AIRs of tests/stark_airs.py the quotient passes the reference's degree check -- which is also what confirms the
factor bound gl_stark_check enforces -- the identity C(zeta) = Z_H(zeta) t(zeta) holds at an extension point,
and one changed trace cell breaks it."""
import numpy as np
import pytest

import stark_airs
import stark_model as sm
from stark_model import P
from vanishing_model import primitive_root

LG_N, NC = 5, 2
U64 = np.uint64


def draw(rng, k):
    return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]


def challenge_sets(rng, air):
    return [[tuple(draw(rng, 2)) for _ in range(NC)] for _ in range(air.q)]


def quotient_of(orc, air, trace, pis, sets, alphas):
    """the model prover's path: Z polynomials, LDEs onto the quotient coset, quotient values, chunks (None: the degree check failed)"""
    zs = sm.permutation_zs(air, NC, trace, sets)[0] if air.pairs else []
    trace_coeffs = orc.ifft(trace)
    zs_coeffs = orc.ifft(np.array(zs, dtype=U64)) if zs else np.zeros((0, 1 << LG_N), dtype=U64)
    trace_q = orc.lde(trace_coeffs, air.qdb)
    zs_q = orc.lde(zs_coeffs, air.qdb) if zs else []
    values = sm.quotient_values(orc, air, NC, LG_N, trace_q, zs_q, sets, alphas, pis)
    return trace_coeffs, zs_coeffs, sm.quotient_chunks(orc, air, NC, LG_N, values)


def identity_at(air, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas):
    from prover_phase_model import eval_ext
    g = primitive_root(LG_N)
    gzeta = (zeta[0] * g % P, zeta[1] * g % P)
    local, nxt = [eval_ext(c, zeta) for c in trace_coeffs], [eval_ext(c, gzeta) for c in trace_coeffs]
    zl, zn = [eval_ext(c, zeta) for c in zs_coeffs], [eval_ext(c, gzeta) for c in zs_coeffs]
    vanishing = sm.vanishing_at(air, NC, LG_N, zeta, local, nxt, pis, alphas, zl, zn, sets)
    return sm.identity_holds(air, NC, LG_N, zeta, vanishing, [eval_ext(c, zeta) for c in chunks])


@pytest.mark.parametrize("name", list(stark_airs.AIRS))
def test_satisfying_trace_passes_the_degree_check_and_the_identity(orc, name):
    air = stark_airs.AIRS[name]
    rng = np.random.Generator(np.random.PCG64(11))
    trace, pis = air.trace(1 << LG_N, seed=1)
    sets, alphas, zeta = challenge_sets(rng, air), draw(rng, NC), tuple(draw(rng, 2))
    trace_coeffs, zs_coeffs, chunks = quotient_of(orc, air, trace, pis, sets, alphas)
    # quotient degree < q n with terms of up to q + 1 trace factors (q under a row filter): the bound gl_stark_check enforces is enough
    longest = max(sum(1 for kind, _ in ops if kind != stark_airs.PUBLIC) for _, terms in air.constraints for _, ops in terms)
    assert longest == (air.q + 1 if name != "fibonacci" else 1)
    assert chunks is not None, "the quotient of a satisfying trace fails trim_to_len(q n)"
    assert chunks.shape == (NC * air.q, 1 << LG_N)
    assert identity_at(air, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas)


@pytest.mark.parametrize("name", list(stark_airs.AIRS))
def test_one_changed_cell_breaks_the_identity(orc, name):
    air = stark_airs.AIRS[name]
    n = 1 << LG_N
    rng = np.random.Generator(np.random.PCG64(12))
    trace, pis = air.trace(n, seed=2)
    sets, alphas, zeta = challenge_sets(rng, air), draw(rng, NC), tuple(draw(rng, 2))
    perm_columns = sorted({c for pair in air.pairs for lr in pair for c in lr})
    cells = [(0, 0), (0, n - 1), (air.num_columns - 1, 0), (air.num_columns - 1, n - 1)] + [(c, r) for c in perm_columns[:4] for r in (0, n - 1)]
    cells += [(int(rng.integers(0, air.num_columns)), int(rng.integers(0, n))) for _ in range(4)]
    if name == "wide":
        cells = cells[:4] + cells[-2:]                   # 130 columns: each evaluation is long
    for col, row in cells:
        bad = trace.copy()
        bad[col, row] = (int(bad[col, row]) + 1) % P
        zs = sm.permutation_zs(air, NC, bad, sets)[0] if air.pairs else []
        trace_coeffs = orc.ifft(bad)
        zs_coeffs = orc.ifft(np.array(zs, dtype=U64)) if zs else np.zeros((0, n), dtype=U64)
        values = sm.quotient_values(orc, air, NC, LG_N, orc.lde(trace_coeffs, air.qdb), orc.lde(zs_coeffs, air.qdb) if zs else [], sets, alphas, pis)
        # without the trim the "quotient" is the interpolant of C / Z_H on the coset: its first q n coefficients stand in for the chunks
        coeffs = orc.coset_ifft(np.array(values, dtype=U64), 7)
        chunks = coeffs[:, :air.q * n].reshape(NC * air.q, n)
        assert not identity_at(air, zeta, trace_coeffs, zs_coeffs, chunks, pis, sets, alphas), \
            "changing cell (column %d, row %d) of %s goes unnoticed" % (col, row, name)


def test_fibonacci_constraints_equal_a_hand_written_evaluation():
    # the five constraints of fibonacci_stark.rs:72-85 written out, not through the term list
    air = stark_airs.fibonacci
    rng = np.random.Generator(np.random.PCG64(13))
    for _ in range(8):
        local, nxt, pub = draw(rng, 4), draw(rng, 4), draw(rng, 3)
        want = [(local[0] - pub[0]) % P, (local[1] - pub[1]) % P, (local[1] - pub[2]) % P, (nxt[0] - local[1]) % P, (nxt[1] - local[0] - local[1]) % P]
        assert sm.constraint_values(sm.Base, air, local, nxt, pub) == want
        alphas, z_last, lf, ll = draw(rng, NC), draw(rng, 1)[0], draw(rng, 1)[0], draw(rng, 1)[0]
        filters = [lf, lf, ll, z_last, z_last]
        accs = [0] * NC
        for c, f in zip(want, filters):
            accs = [(a * al + c * f) % P for a, al in zip(accs, alphas)]
        assert sm.eval_vanishing(sm.Base, stark_airs._air("f", 4, 3, 2, 1, air.constraints, [], None), NC, local, nxt, pub, alphas, z_last, lf, ll) == accs
    assert [f for f, _ in air.constraints] == [stark_airs.FIRST_ROW] * 2 + [stark_airs.LAST_ROW] + [stark_airs.TRANSITION] * 2


@pytest.mark.parametrize("name", ["fibonacci", "cubic", "quartic"])
def test_z_starts_at_one_and_the_quotients_multiply_to_one(name):
    air = stark_airs.AIRS[name]
    rng = np.random.Generator(np.random.PCG64(14))
    trace, _ = air.trace(1 << LG_N, seed=3)
    zs, quotients = sm.permutation_zs(air, NC, trace, challenge_sets(rng, air))
    assert len(zs) == sm.num_zs(air, NC) == {"fibonacci": 2, "cubic": 1, "quartic": 2}[name]
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


def test_lagrange_selectors_on_the_coset_equal_the_closed_forms(orc):
    # L_first(x) = Z_H(x) / (n (x - 1)), L_last(x) = Z_H(x) g^-1 / (n (x - g^-1)): what the kernels use, against the LDE of the selectors
    for qdb in (0, 1, 2):
        lf, ll = sm.lagrange_on_coset(orc, LG_N, qdb)
        n, w, last = 1 << LG_N, primitive_root(LG_N + qdb), pow(primitive_root(LG_N), P - 2, P)
        for i in range(n << qdb):
            x = 7 * pow(w, i, P) % P
            zh = (pow(x, n, P) - 1) % P
            assert lf[i] == zh * pow(n * (x - 1) % P, P - 2, P) % P
            assert ll[i] == zh * last % P * pow(n * (x - last) % P, P - 2, P) % P
