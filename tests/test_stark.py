"""GPU tests of the STARK seam (csrc/stark.hip, csrc/stark_kernels.cuh) against the Python-integer model tests/stark_model.py, itself
pinned by tests/test_stark_model.py, on the AIRs of tests/stark_airs.py under num_challenges 1 to 4 (test_stark_model.py's matrix guard
holds the shapes the cases below rely on).  A case without a count in its name runs the standard configuration's two.

degree_bits 5: 32 rows, less than a wave and one partial segment of the scan, the reference test's size; 12: 4096 rows cross the
2048-row segment of the scan, and the quotient kernel runs 16 to 64 blocks.
"""
import copy

import numpy as np
import pytest

import stark_airs
import stark_model as sm
from stark_model import P
from test_quotient_model import EDGES, edge_targets
from vanishing_model import primitive_root

pytestmark = pytest.mark.gpu
U64 = np.uint64
NC = 2
VARIANTS = ("random", "edges", "non-canonical")
EDGE_CHALLENGES = [0, 1, P - 1, 2**32]
NON_CANONICAL = [P + 3, 2**64 - 1]


def config_of(p, air, nc=NC):
    c = p.StarkConfig.standard_fast_config()
    assert c.num_challenges == NC
    c.num_challenges, c.rate_bits = nc, air.rate_bits
    return c


def case(*args, nc=None):
    """a parametrised case (..., nc); without a count, the standard configuration's two under the plain id"""
    return pytest.param(*args, nc or NC, id="-".join(str(a) for a in args) + ("-nc%d" % nc if nc else ""))


def desc_of(p, air):
    return p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs)


def values_of(variant, rng, k):
    """k words of a variant: seeded draws, the edge list in turn, or non-canonical representatives"""
    if variant == "random":
        return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]
    pool = EDGE_CHALLENGES if variant == "edges" else NON_CANONICAL
    return [pool[(i + int(rng.integers(0, len(pool)))) % len(pool)] for i in range(k)]


def sets_of(variant, rng, air, nc=NC):
    flat = values_of(variant, rng, air.q * nc * 2)
    return [[(flat[2 * (j * nc + c)], flat[2 * (j * nc + c) + 1]) for c in range(nc)] for j in range(air.q)]


def flat_sets(sets):
    return np.array([w for s in sets for ch in s for w in ch], dtype=U64)


# ------------------------------------------------------------------------------- permutation Z by value
def edge_trace_for_the_zs(air, nc, lg_n):
    """-> (the three variants' challenge sets, a trace of EDGES values under which none of them has a zero denominator); needs no GPU"""
    n = 1 << lg_n
    rng = np.random.Generator(np.random.PCG64(500 + lg_n))
    all_sets = {v: sets_of(v, rng, air, nc) for v in VARIANTS}
    edges = np.array(EDGES, dtype=U64)
    batches = sm.permutation_batches(air, nc)
    # columns drawn from the edge operands; where some instance's denominator vanishes for one of the challenge sets, the cells it is made
    # of -- that row of the right-hand columns of the batch's pairs -- are drawn again.  (Drawing the whole row again cannot converge on 33
    # single-column pairs: every gamma of the edge pool is minus an edge operand, so a row is free of zeros with probability (9/11)^33.)
    trace = edges[rng.integers(0, len(EDGES), size=(air.num_columns, n))]
    for _ in range(64):
        bad = np.zeros(n, dtype=bool)
        for sets in all_sets.values():
            for batch, (_, den) in zip(batches, sm.permutation_num_den(air, nc, trace, sets)):
                zero = np.array([d == 0 for d in den])
                if zero.any():
                    bad |= zero
                    cols = sorted({rhs for pair, _, _ in batch for _, rhs in air.pairs[pair]})
                    trace[np.ix_(cols, np.flatnonzero(zero))] = edges[rng.integers(0, len(EDGES), size=(len(cols), int(zero.sum())))]
        if not bad.any():
            break
    assert not bad.any(), "could not arrange the edge rows so that no denominator is zero"
    assert np.isin(trace, edges).all()
    return all_sets, trace


Z_CASES = [case("cubic", 5), case("quartic", 5), case("cubic", 12), case("quartic", 12),
           case("pairs33", 5, nc=2), case("pairs33", 8, nc=2),     # 66 Zs: the second block of k_stark_seg_scan
           case("pairs33", 5, nc=4),                               # 132 Zs: three blocks
           case("longpair", 5, nc=3), case("longpair", 12, nc=3),  # beta^63; three instances in two Zs, the last batch partial; two segments
           case("nonic", 5, nc=3), case("linear", 5, nc=1)]


@pytest.mark.parametrize("name,lg_n,nc", Z_CASES)
def test_permutation_zs_equal_the_model_at_every_word(gpu, orc, name, lg_n, nc):
    p, ctx = gpu
    air = stark_airs.AIRS[name]
    n = 1 << lg_n
    all_sets, trace = edge_trace_for_the_zs(air, nc, lg_n)
    stark = p.Stark(desc_of(p, air), config_of(p, air, nc), lg_n, ctx=ctx)
    for variant, sets in all_sets.items():
        zs_b = stark.permutation_zs(trace, flat_sets(sets))
        want, _ = sm.permutation_zs(air, nc, trace, sets)
        assert zs_b.ncols == sm.num_zs(air, nc) and zs_b.degree == n
        got = orc.fft(zs_b.polynomials)                              # the committed polynomials back on H
        bad_words = np.argwhere(got != np.array(want, dtype=U64))
        assert not len(bad_words), "%s challenges: %d words differ, first (Z, row) %s" % (variant, len(bad_words), bad_words[:4].tolist())


def test_a_zero_denominator_is_refused_not_divided_by(gpu):
    # gamma + rhs = 0 on one row: the reference panics inverting zero; the library answers GL_ERR_ARG and names it
    p, ctx = gpu
    air = stark_airs.cubic
    trace, _ = air.trace(32, seed=5)
    sets = [[(1, 5), (1, 5)], [(1, 5), (1, 5)]]
    trace[4, 7], trace[5, 7] = P - 5, 0                              # rhs columns of the one pair: gamma + c + beta d = 0 on row 7
    stark = p.Stark(desc_of(p, air), config_of(p, air), 5, ctx=ctx)
    with pytest.raises(p.Plonky2Mi355xError, match="permutation denominator is zero") as e:
        stark.permutation_zs(trace, flat_sets(sets))
    assert e.value.code == 1


# ------------------------------------------------------------------------------- quotient by value at every coset point
def through_points(orc, targets, lg_n, rate_bits, k):
    """the value columns (on H_n) of the polynomials of degree < n that take `targets` on the LDE points i = k (mod 2^rate_bits)"""
    shift = 7 * pow(primitive_root(lg_n + rate_bits), k, P) % P
    return orc.fft(orc.coset_ifft(targets, shift))


def variant_of(air, variant, rng):
    """the AIR with its coefficients replaced by a variant's (it need not be satisfiable: the values are compared, not a proof)"""
    a = copy.copy(air)
    a.constraints = [(f, [(c if variant == "random" and rng.integers(0, 2) else values_of(variant, rng, 1)[0], ops) for c, ops in terms]) for f, terms in air.constraints]
    return a


@pytest.mark.parametrize("name,lg_n,nc", [
    case("fibonacci", 5), case("cubic", 5), case("quartic", 5), case("wide", 5), case("quartic", 12), case("wide", 12),
    case("fibonacci", 5, nc=1), case("quartic", 5, nc=3), case("quintic", 5, nc=4), case("sextic", 5, nc=3), case("nonic", 5, nc=4), case("nonic", 5, nc=1),
    case("linear", 5, nc=2), case("longpair", 5, nc=3), case("manyfactors", 5, nc=2), case("nopublic", 5, nc=1),
    case("nonic", 9, nc=3)])       # size 4096: both halves of the two-level power table, and `next` wraps at the last 8 points
def test_quotient_values_equal_the_model_at_every_coset_point(gpu, orc, name, lg_n, nc):
    p, ctx = gpu
    base = stark_airs.AIRS[name]
    n, step = 1 << lg_n, 1 << (base.rate_bits - base.qdb)
    size, nz = n << base.qdb, sm.num_zs(base, nc)
    if name == "quintic":
        assert step == 2 and base.qdb == 2           # every second LDE point, four values of 1 / Z_H
    if (name, lg_n) == ("nonic", 9):
        assert size == 4096 and base.qdb == 3
    rng = np.random.Generator(np.random.PCG64(700 + lg_n))
    k = step * int(rng.integers(0, 1 << base.qdb))                   # a multiple of step: the quotient coset sees the edge rows
    edge_points = np.arange(k, n << base.rate_bits, 1 << base.rate_bits)
    t_trace = edge_targets(rng, base.num_columns, n)
    config = config_of(p, base, nc)
    trace_b = p.PolynomialBatch.from_values(list(through_points(orc, t_trace, lg_n, base.rate_bits, k)), base.rate_bits, False, config.cap_height, ctx=ctx)
    trace_lde = trace_b.lde_values()
    assert (trace_lde[:, edge_points] == t_trace).all()
    zs_b, zs_lde = None, np.zeros((0, n << base.rate_bits), dtype=U64)
    if nz:
        zs_b = p.PolynomialBatch.from_values(list(through_points(orc, edge_targets(rng, nz, n), lg_n, base.rate_bits, k)), base.rate_bits, False, config.cap_height, ctx=ctx)
        zs_lde = zs_b.lde_values()
    for variant in VARIANTS:
        air = variant_of(base, variant, rng)
        stark = p.Stark(desc_of(p, air), config, lg_n, ctx=ctx)
        sets = sets_of(variant, rng, air, nc) if nz else None
        alphas, pis = values_of(variant, rng, nc), values_of(variant, rng, air.num_public_inputs)
        got = stark.quotient_values(trace_b, zs_b, flat_sets(sets) if nz else None, alphas, pis)
        assert got.shape == (nc, size)
        want = np.array(sm.quotient_values(orc, air, nc, lg_n, trace_lde[:, ::step], zs_lde[:, ::step], sets, alphas, pis), dtype=U64)
        bad = np.argwhere(got != want)
        assert not len(bad), "%s at 2^%d, %s variant: %d of %d words differ, first (challenge, point) %s" % (name, lg_n, variant, len(bad), nc * size, bad[:4].tolist())
        # the wrap-around of `next` at the last 2^qdb points is part of the comparison; it reads the first points' rows
        assert (1 << base.qdb) <= size


# ------------------------------------------------------------------------------- quotient polynomials
def model_prover(orc, air, nc, lg_n, trace, pis, sets, alphas):
    """the model's Z values and quotient chunks of a trace (None where trim_to_len fails)"""
    zs = sm.permutation_zs(air, nc, trace, sets)[0] if air.pairs else []
    trace_coeffs = orc.ifft(trace)
    zs_coeffs = orc.ifft(np.array(zs, dtype=U64)) if zs else np.zeros((0, 1 << lg_n), dtype=U64)
    values = sm.quotient_values(orc, air, nc, lg_n, orc.lde(trace_coeffs, air.qdb), orc.lde(zs_coeffs, air.qdb) if zs else [], sets, alphas, pis)
    return zs, trace_coeffs, zs_coeffs, sm.quotient_chunks(orc, air, nc, lg_n, values)


def quotient_polys_and_a_changed_cell(gpu, orc, air, nc, lg_n=5):
    """the chunks of a satisfying trace against the model's -> (the stark, the trace with one cell changed, its public inputs, the challenges)"""
    p, ctx = gpu
    rng = np.random.Generator(np.random.PCG64(900))
    trace, pis = air.trace(1 << lg_n, seed=4)
    sets, alphas = sets_of("random", rng, air, nc), values_of("random", rng, nc)
    stark = p.Stark(desc_of(p, air), config_of(p, air, nc), lg_n, ctx=ctx)
    trace_b = stark.commit_trace(list(trace))
    zs_b = stark.permutation_zs(trace, flat_sets(sets))
    chunks = model_prover(orc, air, nc, lg_n, trace, pis, sets, alphas)[3]
    assert chunks is not None
    q_b = stark.quotient_polys(trace_b, zs_b, flat_sets(sets), alphas, pis)
    assert q_b.ncols == nc * air.q and (q_b.polynomials == chunks).all()
    bad = trace.copy()
    bad[0, 9] = (int(bad[0, 9]) + 1) % P
    return stark, bad, pis, sets, alphas


def refused_through_the_trim(p, stark, bad, pis, sets, alphas):
    with pytest.raises(p.Plonky2Mi355xError, match="does not satisfy the constraints") as e:
        stark.quotient_polys(stark.commit_trace(list(bad)), stark.permutation_zs(bad, flat_sets(sets)), flat_sets(sets), alphas, pis)
    assert e.value.code == 1
    with pytest.raises(p.Plonky2Mi355xError, match="does not satisfy the constraints") as e:
        stark.prove(bad, pis)
    assert e.value.code == 1


def test_quotient_polys_equal_the_model_and_refuse_a_broken_trace(gpu, orc):
    air = stark_airs.quartic
    assert NC * air.q == 6
    # one cell changed: q = 3 is no power of two, so the trim sees the quotient's degree; the one-call prover refuses the same way
    refused_through_the_trim(gpu[0], *quotient_polys_and_a_changed_cell(gpu, orc, air, NC))


def test_quotient_polys_of_five_chunks_equal_the_model_and_refuse_a_broken_trace(gpu, orc):
    # q = 5 under qdb = 3: the trim checks 3 n coefficients per challenge and quotient_commit keeps 5 n of 8 n, three times
    air = stark_airs.sextic
    assert (air.q, air.qdb) == (5, 3)
    refused_through_the_trim(gpu[0], *quotient_polys_and_a_changed_cell(gpu, orc, air, 3))


def test_quotient_polys_of_eight_chunks_equal_the_model_and_the_verifier_rejects_a_broken_trace(gpu, orc):
    # q = 8 fills the coset: nothing to trim, the prover cannot see the changed cell; the identity at zeta does (as for fibonacci below)
    air = stark_airs.nonic
    assert (air.q, air.qdb) == (8, 3)
    stark, bad, pis, _, _ = quotient_polys_and_a_changed_cell(gpu, orc, air, 4)
    trace, _ = air.trace(32, seed=4)
    assert stark.verify(stark.prove(trace, pis)) == (True, "", 0)
    ok, why, code = stark.verify(stark.prove(bad, pis))
    assert (ok, code) == (False, sm.VANISHING) and "anishing" in why


def test_a_broken_fibonacci_trace_yields_a_proof_the_verifier_rejects(gpu):
    # q = 1: nothing to trim, the prover cannot see the broken transition; the identity at zeta does
    p, ctx = gpu
    desc, generate = p.fibonacci_stark(32)
    stark = p.Stark(desc, p.StarkConfig.standard_fast_config(), 5, ctx=ctx)
    trace = generate(0, 1)
    pis = [0, 1, int(trace[1, 31])]
    assert stark.verify(stark.prove(trace, pis)) == (True, "", 0)
    trace[1, 9] += 1
    ok, why, code = stark.verify(stark.prove(trace, pis))
    assert (ok, code) == (False, sm.VANISHING) and "anishing" in why


# ------------------------------------------------------------------------------- whole proofs
def check_whole_proof(p, orc, air, nc, lg_n, hasher, stark, proof, trace, pis, max_queries=None):
    from prover_phase_model import eval_ext
    from test_fri_openings import model_challenger, verify_path_of
    params = stark.params
    assert len(proof) == stark.proof_size
    pp = sm.ParsedStarkProof(air, nc, params, proof)
    assert pp.public_inputs == [int(v) % P for v in pis]
    sets, alphas, zeta = sm.replay(air, nc, pp, model_challenger(orc, hasher))
    assert len(alphas) == nc and len(pp.quotient) == nc * air.q and len(pp.zs) == sm.num_zs(air, nc)
    zs, trace_coeffs, zs_coeffs, chunks = model_prover(orc, air, nc, lg_n, trace, pis, sets, alphas)
    assert chunks is not None
    if hasher == "poseidon":
        cap = lambda cols, values: orc.batch(cols, params.rate_bits, params.cap_height, from_values=values).cap.tolist()       # noqa: E731
    else:                           # the oracle library commits under Poseidon only: the Keccak Merkle model of test_keccak.py over the oracle's LDE
        import test_keccak
        lgN = lg_n + params.rate_bits
        order = [int(format(i, "0%db" % lgN)[::-1], 2) for i in range(1 << lgN)]      # leaf i of the tree is natural LDE row bitrev(i)

        def cap(cols, values):
            lde = orc.lde(orc.ifft(cols) if values else np.asarray(cols, dtype=U64), params.rate_bits)
            return test_keccak.ModelTree(lde.T[order]).cap(params.cap_height).tolist()
    assert pp.trace_cap == cap(trace, True) and pp.quotient_cap == cap(chunks, False)
    if air.pairs:
        assert pp.zs_cap == cap(np.array(zs, dtype=U64), True)
    g = primitive_root(lg_n)
    gzeta = (zeta[0] * g % P, zeta[1] * g % P)
    assert pp.local == [eval_ext(c, zeta) for c in trace_coeffs] and pp.next == [eval_ext(c, gzeta) for c in trace_coeffs]
    assert pp.zs == [eval_ext(c, zeta) for c in zs_coeffs] and pp.zs_next == [eval_ext(c, gzeta) for c in zs_coeffs]
    assert pp.quotient == [eval_ext(c, zeta) for c in chunks]
    seen = {}
    assert sm.verify(air, nc, params, proof, model_challenger(orc, hasher), verify_path_of(orc, hasher), max_queries=max_queries, trace=seen) == sm.fom.ACCEPTED
    assert (seen["zeta"], seen["alphas"]) == (zeta, alphas)           # the model transcript's, which the openings above were checked at
    assert stark.verify(proof) == (True, "", 0)


@pytest.mark.parametrize("name,lg_n,hasher,nc", [
    case("fibonacci", 5, "poseidon"), case("fibonacci", 7, "poseidon"), case("fibonacci", 12, "poseidon"), case("cubic", 7, "poseidon"),
    case("quartic", 7, "poseidon"), case("wide", 5, "poseidon"), case("fibonacci", 7, "keccak"),
    case("fibonacci", 5, "poseidon", nc=1), case("quartic", 7, "poseidon", nc=3), case("nonic", 5, "poseidon", nc=4), case("sextic", 7, "poseidon", nc=3),
    case("pairs33", 5, "poseidon", nc=2), case("longpair", 5, "poseidon", nc=3), case("nonic", 5, "keccak", nc=3)])
def test_whole_proof(gpu, orc, name, lg_n, hasher, nc):
    p, ctx = gpu
    air = stark_airs.AIRS[name]
    trace, pis = air.trace(1 << lg_n, seed=6)
    stark = p.Stark(desc_of(p, air), config_of(p, air, nc), lg_n, hasher=hasher, ctx=ctx)
    assert len(stark.params.reduction_arity_bits) == {5: 0, 7: 1, 12: 2}[lg_n]
    proof = stark.prove(trace, pis)
    check_whole_proof(p, orc, air, nc, lg_n, hasher, stark, proof, trace, pis, max_queries=8 if lg_n == 12 else None)
    assert stark.prove(trace, pis) == proof, "two calls on the same input give different bytes"
    d = ctx.alloc(trace.nbytes).upload(trace)
    try:
        assert stark.prove_device(d.ptr, pis) == proof
    finally:
        d.free()


def test_non_canonical_trace_words_give_the_same_proof(gpu):
    # "inputs may be non-canonical": p added to every cell that leaves room for it (all of them here: the values stay below 2^32 - 1)
    p, ctx = gpu
    desc, generate = p.fibonacci_stark(32)
    stark = p.Stark(desc, p.StarkConfig.standard_fast_config(), 5, ctx=ctx)
    trace = generate(0, 1)
    pis = [0, 1, int(trace[1, 31])]
    assert int(trace.max()) < 2**32 - 1
    shifted = trace.copy()
    shifted[:, ::2] += U64(P)
    shifted[1::2, 1::2] += U64(P)
    assert (shifted >= U64(P)).mean() > 0.7 and ((shifted.astype(object) - trace.astype(object)) % P == 0).all()
    want = stark.prove(trace, pis)
    assert stark.prove(shifted, [v + P for v in pis]) == want
    d = ctx.alloc(shifted.nbytes).upload(shifted)
    try:
        assert stark.prove_device(d.ptr, pis) == want
    finally:
        d.free()
    sets = flat_sets(sets_of("non-canonical", np.random.Generator(np.random.PCG64(3)), stark_airs.fibonacci))
    assert (stark.permutation_zs(shifted, sets).polynomials == stark.permutation_zs(trace, sets % U64(P)).polynomials).all()


def test_the_example_binary_proves_verifies_and_rejects(gpu):
    # examples/fibonacci_stark: the reference's test_fibonacci_stark flow in C++ over the C ABI
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])      # a no-op when up to date
    for args, fragment in (([], "32 rows, result 2178309, 0 FRI reductions, proof 24060 bytes (Poseidon)"), (["7", "--keccak"], "128 rows")):
        r = subprocess.run([os.path.join(root, "examples", "fibonacci_stark")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().split("\n")
        assert fragment in lines[0] and lines[1] == "verified" and lines[2].startswith("a changed public input is rejected: vanishing"), r.stdout


def words_bytes(a):
    return np.ascontiguousarray(np.asarray(a, dtype=U64), dtype="<u8").tobytes()


@pytest.mark.parametrize("name,nc", [case("fibonacci"), case("quartic"), case("wide"), case("nonic", nc=3)])
def test_phase_entries_driven_by_the_python_challenger_reproduce_the_one_call_bytes(gpu, name, nc):
    p, ctx = gpu
    air, lg_n = stark_airs.AIRS[name], 7
    trace, pis = air.trace(1 << lg_n, seed=7)
    stark = p.Stark(desc_of(p, air), config_of(p, air, nc), lg_n, ctx=ctx)
    params, nz = stark.params, sm.num_zs(air, nc)
    ch = p.Challenger()
    trace_b = stark.commit_trace(list(trace))
    ch.observe_hashes(trace_b.cap)
    out = words_bytes(trace_b.cap)
    sets, zs_b = None, None
    if nz:
        sets = np.array(ch.get_n_challenges(2 * air.q * nc), dtype=U64)
        zs_b = stark.permutation_zs(trace, sets)
        ch.observe_hashes(zs_b.cap)
        out += words_bytes(zs_b.cap)
    alphas = ch.get_n_challenges(nc)
    q_b = stark.quotient_polys(trace_b, zs_b, sets, alphas, pis)
    ch.observe_hashes(q_b.cap)
    out += words_bytes(q_b.cap)
    zeta = ch.get_n_challenges(2)
    g = primitive_root(lg_n)
    gzeta = [zeta[0] * g % P, zeta[1] * g % P]
    empty = np.zeros((0, 2), dtype=U64)
    local, nxt, quot = trace_b.open_at(zeta), trace_b.open_at(gzeta), q_b.open_at(zeta)
    zl, zn = (zs_b.open_at(zeta), zs_b.open_at(gzeta)) if nz else (empty, empty)
    for part in (local, nxt, zl, zn, quot):
        out += words_bytes(part)
    for part in (local, zl, quot, nxt, zn):                            # FriOpenings order (proof.rs:161-182)
        ch.observe_elements(part)
    model_instance = sm.fri_instance(air, nc, zeta, lg_n)
    instance = p.FriInstance(model_instance.oracles, model_instance.batches)
    out += p.PolynomialBatch.prove_openings(instance, [trace_b] + ([zs_b] if nz else []) + [q_b], ch, params, ctx=ctx)
    out += words_bytes(pis)
    assert out == stark.prove(trace, pis)


def test_eight_threads_with_a_context_each_prove_the_same_bytes(gpu):
    import threading
    p, ctx = gpu
    desc, generate = p.fibonacci_stark(128)
    trace = generate(3, 5)
    pis = [3, 5, int(trace[1, 127])]
    config = p.StarkConfig.standard_fast_config()
    want = p.Stark(desc, config, 7, ctx=ctx).prove(trace, pis)
    got, errors = [None] * 8, []

    def work(i):
        try:
            own = p.Context(0)
            got[i] = p.Stark(desc, config, 7, ctx=own).prove(trace, pis)
        except Exception as e:                                       # noqa: BLE001  (reported below, on the main thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(g == want for g in got)


def test_the_committed_fixture_is_current(gpu):
    import os
    p, ctx = gpu
    desc, generate = p.fibonacci_stark(32)
    trace = generate(0, 1)
    proof = p.Stark(desc, p.StarkConfig.standard_fast_config(), 5, ctx=ctx).prove(trace, [0, 1, int(trace[1, 31])])
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stark_fibonacci_n32.bin"), "rb") as f:
        assert f.read() == proof, "tests/golden/stark_fibonacci_n32.bin is stale: run tools/make_stark_fixture.py on the GPU"


def test_the_committed_nonic_fixture_is_current(gpu):
    import json
    import os
    p, ctx = gpu
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "stark_nonic_n32_nc3.json")) as f:
        meta = json.load(f)
    air, nc = stark_airs.AIRS[meta["air"]], meta["num_challenges"]
    assert (meta["air"], nc, meta["num_rows"], meta["params"]["rate_bits"]) == ("nonic", 3, 32, 3)
    trace, pis = air.trace(meta["num_rows"], seed=meta["trace_seed"])
    assert pis == meta["public_inputs"]
    proof = p.Stark(desc_of(p, air), config_of(p, air, nc), 5, ctx=ctx).prove(trace, pis)
    with open(os.path.join(golden, "stark_nonic_n32_nc3.bin"), "rb") as f:
        assert f.read() == proof, "tests/golden/stark_nonic_n32_nc3.bin is stale: run tools/make_stark_fixture.py nonic on the GPU"


# ------------------------------------------------------------------------------- refusals that need a context
def test_phase_entries_refuse_batches_that_do_not_match(gpu):
    p, ctx = gpu
    air = stark_airs.cubic
    trace, pis = air.trace(32, seed=8)
    config = config_of(p, air)
    stark = p.Stark(desc_of(p, air), config, 5, ctx=ctx)
    sets, alphas = flat_sets(sets_of("random", np.random.Generator(np.random.PCG64(1)), air)), [3, 4]
    trace_b, zs_b = stark.commit_trace(list(trace)), stark.permutation_zs(trace, sets)

    def refused(*args):
        with pytest.raises(p.Plonky2Mi355xError) as e:
            stark.quotient_values(*args)
        return e.value.code
    assert stark.quotient_values(trace_b, zs_b, sets, alphas, pis).shape == (NC, 64)
    assert refused(zs_b, zs_b, sets, alphas, pis) == 1               # a trace batch of another width
    assert refused(trace_b, trace_b, sets, alphas, pis) == 1         # a Z batch of another width
    assert refused(trace_b, None, None, alphas, pis) == 1            # pairs without their Z batch
    other_rate = p.PolynomialBatch.from_values(list(trace), 2, False, config.cap_height, ctx=ctx)
    assert refused(other_rate, zs_b, sets, alphas, pis) == 1
    keccak = p.PolynomialBatch.from_values(list(trace), 1, False, config.cap_height, ctx=ctx, hasher="keccak")
    assert refused(keccak, zs_b, sets, alphas, pis) == 1
    # a description without pairs takes no Z batch and computes no Z polynomials
    wide = p.Stark(desc_of(p, stark_airs.wide), config, 5, ctx=ctx)
    wtrace, wpis = stark_airs.wide.trace(32, seed=8)
    with pytest.raises(p.Plonky2Mi355xError, match="no permutation pairs"):
        wide.permutation_zs(wtrace, np.zeros(4, dtype=U64))
    with pytest.raises(p.Plonky2Mi355xError):
        wide.quotient_values(wide.commit_trace(list(wtrace)), zs_b, np.zeros(4, dtype=U64), alphas, wpis)
    # a stark belongs to the context it was created on
    other = p.Context(0)
    al, pi, out = np.array(alphas, dtype=U64), np.array(pis, dtype=U64), np.empty((NC, 64), dtype=U64)
    with pytest.raises(p.Plonky2Mi355xError, match="another context") as e:
        p.api.check(p.api.lib.gl_stark_quotient_values(other.handle, stark.handle, trace_b.handle, zs_b.handle, sets.ctypes.data, al.ctypes.data, pi.ctypes.data,
                                                       out.ctypes.data))
    assert e.value.code == 1
    # an output buffer below gl_stark_proof_size
    import ctypes
    cols = [np.ascontiguousarray(c) for c in trace]
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    small, k = np.empty(stark.proof_size - 1, dtype=np.uint8), ctypes.c_size_t()
    pi = np.array(pis, dtype=U64)
    assert p.api.lib.gl_stark_prove(ctx.handle, stark.handle, ptrs, pi.ctypes.data, small.ctypes.data, small.size, ctypes.byref(k)) == 1
    assert k.value == stark.proof_size
