"""GPU tests of the memory table (csrc/memory_trace.hip, gl_memory_stark_desc): the device trace against the sequential model of
tests/memory_model.py at all 26 n words of every crafted log of tests/memory_cases.py, from host ops and from device ops; the refusals;
MemoryStark proved end to end from a device-generated trace at 2^5 and 2^12 rows, alone, in DAG form, in a table set behind a
cross-table lookup, and through the batch verifier.  Nothing goes above 2^13 rows."""
import ctypes

import numpy as np
import pytest

import memory_cases as mc
import memory_model as mm
import stark_model as sm
from memory_model import P

pytestmark = pytest.mark.gpu
U64 = np.uint64
GL_ERR_ARG, GL_ERR_UNSUPPORTED = 1, 3
MARKER = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def modelled():
    """name -> the model's trace [26][n], computed once and left unchanged"""
    return {name: np.array(mm.generate_trace(log), dtype=U64) for name, log in mc.CASES.items()}


def device_trace(p, ctx, ops, from_device=False):
    """(rows, [26][rows] after one fill of a buffer full of markers)"""
    d_ops = None
    if from_device:
        raw = np.frombuffer(ops.tobytes(), dtype=U64)               # 56 bytes an op: seven words
        d_ops = ctx.alloc(raw.nbytes).upload(raw)
        trace = p.MemoryTrace(ctx=ctx, device_ptr=d_ops.ptr, num_ops=ops.size)
        d_ops.upload(np.full(raw.size, MARKER, dtype=U64))          # the log is not needed once the handle exists
    else:
        trace = p.MemoryTrace(ops, ctx=ctx)
    n = trace.rows
    d = ctx.alloc(26 * n * 8).upload(np.full((26, n), MARKER, dtype=U64))
    try:
        trace.fill(d.ptr)
        return n, d.download((26, n))
    finally:
        d.free()
        trace.close()
        if d_ops is not None:
            d_ops.free()


@pytest.mark.parametrize("source", ["host-ops", "device-ops"])
def test_fill_equals_the_model_at_every_word_of_every_case(gpu, modelled, source):
    p, ctx = gpu
    for name, log in mc.CASES.items():
        n, got = device_trace(p, ctx, mc.records(log), from_device=source == "device-ops")
        assert n == modelled[name].shape[1], name
        bad = np.argwhere(got != modelled[name])
        assert bad.size == 0, (name, bad[:5].tolist())


def test_fill_equals_the_model_on_random_logs(gpu):
    import test_memory_model as tmm
    p, ctx = gpu
    rng = np.random.Generator(np.random.PCG64(21))
    for k in range(40):
        log = tmm.random_ops(rng, int(rng.integers(1, 60)))
        n, got = device_trace(p, ctx, mc.records(log))
        assert (got == np.array(mm.generate_trace(log), dtype=U64)).all(), k


def test_two_fills_of_one_handle_are_identical(gpu, modelled):
    p, ctx = gpu
    name = "dummies-from-several-pairs-padding-mid-trace"
    trace = p.MemoryTrace(mc.records(mc.CASES[name]), ctx=ctx)
    n = trace.rows
    a, b = ctx.alloc(26 * n * 8), ctx.alloc(26 * n * 8)
    try:
        trace.fill(a.ptr)
        trace.fill(b.ptr)
        trace.fill(a.ptr)                                            # ... and a second time over its own output
        first, second = a.download((26, n)), b.download((26, n))
        assert (first == second).all() and (first == modelled[name]).all()
    finally:
        a.free()
        b.free()
        trace.close()


def test_every_refusal_and_the_columns_are_left_alone(gpu):
    p, ctx = gpu
    from plonky2_demo_amd import _lib
    lib = _lib.lib
    cols = np.full((26, 16), MARKER, dtype=U64)
    d = ctx.alloc(cols.nbytes).upload(cols)
    handle = ctypes.c_void_p()

    def new(ops, num_ops=None, ctx_handle=ctx.handle, out=True):
        handle.value = None
        st = lib.gl_memory_trace_new(ctx_handle, ops.ctypes.data_as(ctypes.c_void_p) if ops is not None else None, ops.size if num_ops is None else num_ops,
                                     ctypes.byref(handle) if out else None)
        assert st == 0 or not handle.value
        return st
    good = mc.records(mc.CASES["three-ops"])
    try:
        assert new(good, ctx_handle=None) == GL_ERR_ARG and new(None, num_ops=3) == GL_ERR_ARG and new(good, out=False) == GL_ERR_ARG
        assert new(good, num_ops=0) == GL_ERR_ARG
        assert lib.gl_memory_trace_new_device(ctx.handle, None, 3, ctypes.byref(handle)) == GL_ERR_ARG
        assert lib.gl_memory_trace_new_device(ctx.handle, d.ptr, 0, ctypes.byref(handle)) == GL_ERR_ARG
        for field in ("filter", "is_read"):
            for bad in (2, 0xFFFFFFFF):
                ops = good.copy()
                ops[field][2] = bad
                assert new(ops) == GL_ERR_ARG, (field, bad)
        for name, log in mc.REFUSED.items():                         # a context or segment step, minus one, that is >= n
            assert new(mc.records(log)) == GL_ERR_ARG, name
            assert "range check" in (lib.gl_last_error() or b"").decode()
        for name, log in mc.TOO_HIGH.items():                        # 2^31 rows asked for by one pair; 2^24 + 1 rows
            assert new(mc.records(log)) == GL_ERR_UNSUPPORTED, name
        assert lib.gl_memory_trace_fill(None, d.ptr) == GL_ERR_ARG
        for name, log in mc.ALLOWED_STEPS.items():
            assert new(mc.records(log)) == 0, name
            assert lib.gl_memory_trace_fill(handle, None) == GL_ERR_ARG
            lib.gl_memory_trace_free(handle)
        assert lib.gl_memory_trace_rows(None) == 0
        assert (d.download(cols.shape) == cols).all(), "a refused call wrote to the columns"
    finally:
        d.free()


# ------------------------------------------------------------------------------- end to end
def as_air(desc):
    from types import SimpleNamespace
    return SimpleNamespace(constraints=desc.constraints, pairs=desc.pairs, q=desc.quotient_degree_factor, qdb=desc.quotient_degree_bits, num_columns=desc.num_columns,
                           num_public_inputs=0, constraint_degree=desc.constraint_degree)


def prove_from_the_device(p, ctx, stark, log):
    trace = p.MemoryTrace(mc.records(log), ctx=ctx)
    assert trace.rows == 1 << stark.degree_bits
    d = ctx.alloc(26 * trace.rows * 8)
    try:
        trace.fill(d.ptr)
        return stark.prove_device(d.ptr, [])
    finally:
        d.free()
        trace.close()


@pytest.mark.parametrize("lg_n", [5, 12])
def test_memory_stark_proved_without_the_trace_leaving_the_device(gpu, orc, lg_n):
    from test_fri_openings import model_challenger, verify_path_of
    p, ctx = gpu
    nc = 2
    desc, config = p.memory_stark(), p.StarkConfig.standard_fast_config()
    air = as_air(desc)
    assert (air.constraint_degree, air.q, config.num_challenges) == (3, 2, nc)
    stark = p.Stark(desc, config, lg_n, ctx=ctx)
    log = mc.end_to_end_log(lg_n)
    queries = 8 if lg_n == 12 else None

    def model_verdict(proof):
        return sm.verify(air, nc, stark.params, proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon"), max_queries=queries)
    proof = prove_from_the_device(p, ctx, stark, log)
    assert stark.verify(proof) == (True, "", 0)
    assert model_verdict(proof) == sm.fom.ACCEPTED
    model_cols = np.array(mm.generate_trace(log), dtype=U64)
    assert model_cols.shape == (26, 1 << lg_n) and model_cols.shape[1] > mm.next_power_of_two(len(log)) // 2
    assert proof == stark.prove(model_cols, [])
    dag = p.Stark(mc.dag_desc(p), config, lg_n, ctx=ctx)
    assert dag.prove(model_cols, []) == proof
    assert dag.verify(proof) == (True, "", 0)


def test_a_read_that_returns_what_was_not_written_generates_and_is_rejected(gpu, orc):
    from test_fri_openings import model_challenger, verify_path_of
    p, ctx = gpu
    desc, config = p.memory_stark(), p.StarkConfig.standard_fast_config()
    stark = p.Stark(desc, config, 5, ctx=ctx)
    bad = prove_from_the_device(p, ctx, stark, mc.mismatched_read())     # q = 2 is a power of two: the prover's trim has nothing to look at
    ok, why, code = stark.verify(bad)
    assert (ok, code) == (False, sm.VANISHING) and "anishing" in why
    assert sm.verify(as_air(desc), 2, stark.params, bad, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon")) == sm.VANISHING


def op_log_table(p, log, lg_n):
    """the looking table of the set: the ops in issue order with a filter column, zero-padded; one constraint, filter (filter - 1)"""
    t = np.zeros((14, 1 << lg_n), dtype=U64)
    for k, o in enumerate(log):
        t[:, k] = [o["filter"], o["is_read"], o["context"], o["segment"], o["virt"]] + o["value"] + [o["timestamp"]]
    desc = p.StarkDesc(14, 0, 3, [(p.GL_STARK_ALL, [(1, [(p.GL_STARK_LOCAL, 0), (p.GL_STARK_LOCAL, 0)]), (P - 1, [(p.GL_STARK_LOCAL, 0)])])])
    return desc, t


def test_a_table_set_of_an_op_log_and_the_memory_table(gpu):
    p, ctx = gpu
    log = mc.end_to_end_log(5)
    n, memory = device_trace(p, ctx, mc.records(log))
    assert n == 32
    log_desc, log_trace = op_log_table(p, log, 5)
    looking = p.TableWithColumns(0, p.CtlColumn.singles(range(1, 14)), p.CtlColumn.single(0))
    looked = p.TableWithColumns(1, p.memory_ctl_data(), p.memory_ctl_filter())
    set_desc = p.StarkSetDesc([(log_desc, 5), (p.memory_stark(), 5)], [p.CrossTableLookup([looking], looked)], p.StarkConfig.standard_fast_config())
    set_desc.check()
    stark_set = p.StarkSet(set_desc, ctx=ctx)
    proof = stark_set.prove([log_trace, memory])
    assert stark_set.verify(proof)[:3] == (True, "", 0)
    # one value limb changed in the log only: both tables still satisfy their own constraints, the lookup does not hold
    k = next(i for i, o in enumerate(log) if o["filter"])
    log_trace[5 + 3, k] ^= U64(1)
    ok, why, code, table = stark_set.verify(stark_set.prove([log_trace, memory]))
    assert (ok, code, table) == (False, p._lib.GL_CHECK_CTL, 2)


def test_the_batch_verifier_gives_the_verdicts_of_the_single_calls(gpu):
    p, ctx = gpu
    stark = p.Stark(p.memory_stark(), p.StarkConfig.standard_fast_config(), 5, ctx=ctx)
    good = prove_from_the_device(p, ctx, stark, mc.end_to_end_log(5))
    bad = prove_from_the_device(p, ctx, stark, mc.mismatched_read())
    tampered = bytearray(good)
    tampered[len(good) // 2] ^= 4
    proofs = [good, bad, bytes(tampered), good, good[:-8], bad, good, bytes(tampered)]
    singles = [stark.verify(pr) for pr in proofs]
    assert [s[0] for s in singles] == [True, False, False, True, False, False, True, False]
    got = stark.batch_verifier(max_batch=8).verify(proofs)
    assert [(ok, code) for ok, _, code in got] == [(ok, code) for ok, _, code in singles]
