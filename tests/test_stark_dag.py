"""GPU tests of STARK constraints as an expression DAG (csrc/stark_dag.hip, csrc/stark_dag_kernels.cuh): k_stark_quotient_dag and the
host interpreter against the term-list path where a term list states the same AIR -- word for word and byte for byte -- and against the
Python-integer model tests/stark_dag_model.py, itself pinned by tests/test_stark_dag_model.py, where none can (tests/stark_dag_airs.py).
The machinery -- edge operands, challenge variants, interpolation through edge points, the transcript replay -- is tests/test_stark.py's.

Sizes are 2^5 rows unless a case says otherwise: less than a wave of the 64-thread workgroups at q = 1, four workgroups at q = 8.
"""
import copy
import json
import os

import numpy as np
import pytest

import stark_airs
import stark_dag_airs as da
import stark_dag_model as dm
import stark_model as sm
import test_stark as ts
from stark_model import P
from test_quotient_model import edge_targets
from vanishing_model import primitive_root

pytestmark = pytest.mark.gpu
U64 = np.uint64


def dag_stark(gpu, dag, nc, lg_n=5, hasher="poseidon"):
    p, ctx = gpu
    return p.Stark(dm.desc_of(p, dag), ts.config_of(p, dag, nc), lg_n, hasher=hasher, ctx=ctx)


# ------------------------------------------------------------------------------- the twelve converted AIRs: the term-list path's words and bytes
@pytest.mark.parametrize("nc", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(da.CONVERTED))
def test_a_converted_air_gives_the_term_lists_quotient_words_and_proof_bytes(gpu, name, nc):
    p, ctx = gpu
    air, dag = stark_airs.AIRS[name], da.CONVERTED[name]
    terms, nodes = p.Stark(ts.desc_of(p, air), ts.config_of(p, air, nc), 5, ctx=ctx), dag_stark(gpu, dag, nc)
    assert nodes.proof_size == terms.proof_size
    trace, pis = air.trace(32, seed=2)
    rng = np.random.Generator(np.random.PCG64(300 + nc))
    nz = sm.num_zs(air, nc)
    sets = ts.flat_sets(ts.sets_of("random", rng, air, nc)) if nz else None
    alphas = ts.values_of("random", rng, nc)
    trace_b = terms.commit_trace(list(trace))
    zs_b = terms.permutation_zs(trace, sets) if nz else None
    want = terms.quotient_values(trace_b, zs_b, sets, alphas, pis)
    got = nodes.quotient_values(trace_b, zs_b, sets, alphas, pis)      # the same batches
    bad = np.argwhere(got != want)
    assert not len(bad), "%s, %d challenges: %d of %d words differ, first (challenge, point) %s" % (name, nc, len(bad), want.size, bad[:4].tolist())
    if nz:
        assert (nodes.permutation_zs(trace, sets).polynomials == zs_b.polynomials).all()
    proof = terms.prove(trace, pis)
    assert nodes.prove(trace, pis) == proof, "the DAG's proof differs from the term list's"
    assert nodes.verify(proof) == (True, "", 0) == terms.verify(proof)


def test_a_converted_air_on_a_coset_of_4096_points_gives_the_term_lists_words(gpu):
    # both halves of the two-level power table, 64 workgroups, and `next` wraps at the last 8 points
    p, ctx = gpu
    air, dag, nc, lg_n = stark_airs.nonic, da.CONVERTED["nonic"], 3, 9
    assert (1 << lg_n) << air.qdb == 4096
    terms, nodes = p.Stark(ts.desc_of(p, air), ts.config_of(p, air, nc), lg_n, ctx=ctx), dag_stark(gpu, dag, nc, lg_n)
    trace, pis = air.trace(1 << lg_n, seed=2)
    rng = np.random.Generator(np.random.PCG64(309))
    sets, alphas = ts.flat_sets(ts.sets_of("random", rng, air, nc)), ts.values_of("non-canonical", rng, nc)
    trace_b = terms.commit_trace(list(trace))
    zs_b = terms.permutation_zs(trace, sets)
    want = terms.quotient_values(trace_b, zs_b, sets, alphas, pis)
    assert want.shape == (nc, 4096) and (nodes.quotient_values(trace_b, zs_b, sets, alphas, pis) == want).all()


# ------------------------------------------------------------------------------- the DAGs' own AIRs against the model at every coset point
def variant_of(dag, variant, rng):
    """the DAG with its constants replaced by a variant's (it need not be satisfiable: the values are compared, not a proof)"""
    d = copy.copy(dag)
    d.constants = [c if variant == "random" and rng.integers(0, 2) else ts.values_of(variant, rng, 1)[0] for c in dag.constants]
    return d


OWN_CASES = [("sbox2", 2), ("sbox2", 4), ("at_cap128", 1), ("at_cap128", 3), ("alias", 2), ("operands", 3)] + [(name, 2) for name in da.BOUND]


@pytest.mark.parametrize("name,nc", OWN_CASES, ids=["%s-nc%d" % c for c in OWN_CASES])
def test_quotient_values_equal_the_model_at_every_coset_point(gpu, orc, name, nc):
    p, ctx = gpu
    base, lg_n = da.OWN[name], 5
    n, step = 1 << lg_n, 1 << (base.rate_bits - base.qdb)
    size = n << base.qdb
    rng = np.random.Generator(np.random.PCG64(800 + nc))
    k = step * int(rng.integers(0, 1 << base.qdb))
    edge_points = np.arange(k, n << base.rate_bits, 1 << base.rate_bits)
    t_trace = edge_targets(rng, base.num_columns, n)
    config = ts.config_of(p, base, nc)
    trace_b = p.PolynomialBatch.from_values(list(ts.through_points(orc, t_trace, lg_n, base.rate_bits, k)), base.rate_bits, False, config.cap_height, ctx=ctx)
    trace_lde = trace_b.lde_values()
    assert (trace_lde[:, edge_points] == t_trace).all()              # the quotient coset sees rows of edge operands
    for variant in ts.VARIANTS:
        dag = variant_of(base, variant, rng)
        stark = p.Stark(dm.desc_of(p, dag), config, lg_n, ctx=ctx)
        alphas, pis = ts.values_of(variant, rng, nc), ts.values_of(variant, rng, dag.num_public_inputs)
        got = stark.quotient_values(trace_b, None, None, alphas, pis)
        assert got.shape == (nc, size)
        want = np.array(dm.quotient_values(orc, dag, nc, lg_n, trace_lde[:, ::step], [], None, alphas, pis), dtype=U64)
        bad = np.argwhere(got != want)
        assert not len(bad), "%s, %s variant: %d of %d words differ, first (challenge, point) %s" % (name, variant, len(bad), nc * size, bad[:4].tolist())


def test_the_sibling_one_value_above_the_live_cap_is_refused_at_create(gpu):
    p, ctx = gpu
    with pytest.raises(p.Plonky2Mi355xError, match="128 values live") as e:
        dag_stark(gpu, da.at_cap(129), 2)
    assert e.value.code == 1


@pytest.mark.parametrize("name", ["at_cap128", "alias", "operands"] + list(da.BOUND))
def test_a_satisfying_trace_is_proved_and_verified(gpu, orc, name):
    from test_fri_openings import model_challenger, verify_path_of
    dag = da.OWN[name]
    stark = dag_stark(gpu, dag, 2)
    trace, pis = dag.trace(32, seed=5)
    proof = stark.prove(trace, pis)
    assert stark.verify(proof) == (True, "", 0)
    assert dm.verify(dag, 2, stark.params, proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == 0


# ------------------------------------------------------------------------------- whole proofs of sbox2
def model_prover(orc, dag, nc, lg_n, trace, pis, alphas):
    trace_coeffs = orc.ifft(trace)
    values = dm.quotient_values(orc, dag, nc, lg_n, orc.lde(trace_coeffs, dag.qdb), [], None, alphas, pis)
    return trace_coeffs, sm.quotient_chunks(orc, dag, nc, lg_n, values)


def check_whole_proof(p, orc, dag, nc, lg_n, hasher, stark, proof, trace, pis):
    """test_stark.check_whole_proof for a table without pairs in DAG form: caps rebuilt, openings recomputed, transcript replayed"""
    from prover_phase_model import eval_ext
    from test_fri_openings import model_challenger, verify_path_of
    params = stark.params
    assert len(proof) == stark.proof_size
    pp = sm.ParsedStarkProof(dag, nc, params, proof)
    assert pp.public_inputs == [int(v) % P for v in pis]
    sets, alphas, zeta = sm.replay(dag, nc, pp, model_challenger(orc, hasher))
    assert sets is None and len(alphas) == nc and len(pp.quotient) == nc * dag.q
    trace_coeffs, chunks = model_prover(orc, dag, nc, lg_n, trace, pis, alphas)
    assert chunks is not None
    if hasher == "poseidon":
        cap = lambda cols, values: orc.batch(cols, params.rate_bits, params.cap_height, from_values=values).cap.tolist()       # noqa: E731
    else:
        import test_keccak
        lgN = lg_n + params.rate_bits
        order = [int(format(i, "0%db" % lgN)[::-1], 2) for i in range(1 << lgN)]

        def cap(cols, values):
            lde = orc.lde(orc.ifft(cols) if values else np.asarray(cols, dtype=U64), params.rate_bits)
            return test_keccak.ModelTree(lde.T[order]).cap(params.cap_height).tolist()
    assert pp.trace_cap == cap(trace, True) and pp.quotient_cap == cap(chunks, False)
    g = primitive_root(lg_n)
    gzeta = (zeta[0] * g % P, zeta[1] * g % P)
    assert pp.local == [eval_ext(c, zeta) for c in trace_coeffs] and pp.next == [eval_ext(c, gzeta) for c in trace_coeffs]
    assert pp.quotient == [eval_ext(c, zeta) for c in chunks]
    seen = {}
    assert dm.verify(dag, nc, params, proof, model_challenger(orc, hasher), verify_path_of(orc, hasher), trace=seen) == sm.fom.ACCEPTED
    assert (seen["zeta"], seen["alphas"]) == (zeta, alphas)
    assert stark.verify(proof) == (True, "", 0)
    assert p.stark_dag_verify(stark.desc, stark.config, lg_n, proof, hasher=hasher) == (True, "", 0)


@pytest.mark.parametrize("hasher", ["poseidon", "keccak"])
def test_whole_proof_of_sbox2(gpu, orc, hasher):
    p, ctx = gpu
    dag, nc, lg_n = da.sbox2, 2, 5
    stark = dag_stark(gpu, dag, nc, lg_n, hasher)
    trace, pis = dag.trace(1 << lg_n, seed=6)
    proof = stark.prove(trace, pis)
    check_whole_proof(p, orc, dag, nc, lg_n, hasher, stark, proof, trace, pis)
    assert stark.prove(trace, pis) == proof, "two calls on the same input give different bytes"
    # one changed cell: q = 8 fills the coset, nothing to trim; the identity at zeta sees it
    bad = trace.copy()
    bad[3, 9] = (int(bad[3, 9]) + 1) % P
    ok, why, code = stark.verify(stark.prove(bad, pis))
    assert (ok, code) == (False, sm.VANISHING) and "anishing" in why
    d = ctx.alloc(trace.nbytes).upload(trace)
    try:
        assert stark.prove_device(d.ptr, pis) == proof
    finally:
        d.free()
    # "inputs may be non-canonical": a word below 2^32 - 1 has a second representative, and a satisfying trace of random words has next to
    # none, so half the cells are cut down to 31 bits first (at q = 8 the prover does not look whether the trace satisfies the AIR)
    low = trace.copy()
    low[:, ::2] %= U64(1 << 31)
    other = low.copy()
    other[:, ::2] += U64(P)
    assert (other != low).any() and stark.prove(other, [v % (1 << 31) + P for v in pis]) == stark.prove(low, [v % (1 << 31) for v in pis])


def test_phase_entries_driven_by_the_python_challenger_reproduce_the_one_call_bytes_of_sbox2(gpu):
    p, ctx = gpu
    dag, nc, lg_n = da.sbox2, 2, 7
    trace, pis = dag.trace(1 << lg_n, seed=7)
    stark = dag_stark(gpu, dag, nc, lg_n)
    ch = p.Challenger()
    trace_b = stark.commit_trace(list(trace))
    ch.observe_hashes(trace_b.cap)
    out = ts.words_bytes(trace_b.cap)
    alphas = ch.get_n_challenges(nc)
    q_b = stark.quotient_polys(trace_b, None, None, alphas, pis)
    assert q_b.ncols == nc * dag.q
    ch.observe_hashes(q_b.cap)
    out += ts.words_bytes(q_b.cap)
    zeta = ch.get_n_challenges(2)
    g = primitive_root(lg_n)
    local, nxt, quot = trace_b.open_at(zeta), trace_b.open_at([zeta[0] * g % P, zeta[1] * g % P]), q_b.open_at(zeta)
    for part in (local, nxt, quot):
        out += ts.words_bytes(part)
    for part in (local, quot, nxt):                                    # FriOpenings order (proof.rs:161-182)
        ch.observe_elements(part)
    model_instance = sm.fri_instance(dag, nc, zeta, lg_n)
    out += p.PolynomialBatch.prove_openings(p.FriInstance(model_instance.oracles, model_instance.batches), [trace_b, q_b], ch, stark.params, ctx=ctx)
    out += ts.words_bytes(pis)
    assert out == stark.prove(trace, pis)


# ------------------------------------------------------------------------------- a table set with one table as a DAG
def test_a_set_with_its_mul_table_as_a_dag_gives_the_all_term_list_sets_bytes(gpu, orc):
    import stark_ctl_airs as ca
    import stark_ctl_model as cm
    import test_stark_ctl as tc
    from test_fri_openings import verify_path_of
    p, ctx = gpu
    lgs, nc = [5, 6, 5], 2
    config = ca.config(p, nc)
    plain, mixed = p.StarkSet(da.api_set(p, lgs, config, dag_tables=()), ctx=ctx), p.StarkSet(da.api_set(p, lgs, config), ctx=ctx)
    assert isinstance(mixed.desc.tables[ca.MUL][0], p.StarkDagDesc) and mixed.counts == plain.counts and mixed.proof_size == plain.proof_size
    traces = ca.traces(lgs, seed=7)
    proof = plain.prove(traces)
    assert mixed.prove(traces) == proof, "the set with a DAG table proves other bytes"
    assert mixed.verify(proof) == (True, "", 0, 3) == plain.verify(proof)
    params = [mixed.desc.fri_params(t) for t in range(3)]
    assert cm.verify_set(ca.TABLES, ca.LOOKUPS, nc, params, proof, tc.model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == (0, 3)
    # the phase entry of the DAG table, CTL pass after the DAG quotient, word for word
    rng = np.random.Generator(np.random.PCG64(5))
    ctl, alphas = ts.values_of("random", rng, 2 * nc), ts.values_of("random", rng, nc)
    trace_b = p.PolynomialBatch.from_values(list(traces[ca.MUL]), config.rate_bits, False, config.cap_height, ctx=ctx)
    zs_b = plain.zs(ca.MUL, traces[ca.MUL], None, ctl)
    want = plain.quotient_values(ca.MUL, trace_b, zs_b, None, ctl, alphas, [])
    assert (mixed.quotient_values(ca.MUL, trace_b, zs_b, None, ctl, alphas, []) == want).all()
    # the inconsistent system: every table's own proof verifies, the product across tables fails
    removed = mixed.prove(ca.remove_one_looked_row(ca.traces(lgs, seed=8)))
    ok, why, code, table = mixed.verify(removed)
    assert (ok, code, table) == (False, p._lib.GL_CHECK_CTL, 3) and "ross-table" in why


# ------------------------------------------------------------------------------- the committed fixture
def test_the_committed_fixture_is_current(gpu):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "stark_dag_sbox2_n32.json")) as f:
        meta = json.load(f)
    dag, nc = da.EVERY[meta["air"]], meta["num_challenges"]
    assert (meta["air"], nc, meta["num_rows"], meta["params"]["rate_bits"]) == ("sbox2", 2, 32, 3)
    trace, pis = dag.trace(meta["num_rows"], seed=meta["trace_seed"])
    assert pis == meta["public_inputs"]
    proof = dag_stark(gpu, dag, nc).prove(trace, pis)
    with open(os.path.join(golden, "stark_dag_sbox2_n32.bin"), "rb") as f:
        assert f.read() == proof, "tests/golden/stark_dag_sbox2_n32.bin is stale: run tools/make_stark_dag_fixture.py on the GPU"
