"""GPU tests of gl_stark_lookup_columns (csrc/stark_lookup.hip): permuted_cols (evm/src/lookup.rs:65-127) on the device against the
sequential model of tests/lookup_model.py, all 2 n output words of every crafted case of tests/lookup_cases.py; calls of many lookups;
the refusals; and a range-checked table proved end to end from a device trace."""
import ctypes

import numpy as np
import pytest

import lookup_cases as lc
import lookup_model as lm
import stark_model as sm
from lookup_model import P

pytestmark = pytest.mark.gpu
U64 = np.uint64
GL_ERR_ARG = 1
# The scans run over the 2 n merge places in segments of lc.SEG = 2048 places: n = 2^10 is one segment, 2^11 two, 2^12 four; 256 is one
# workgroup of the per-row launches, 512 two.
SIZES = (2, 32, 256, 512, 1 << 10, 1 << 11, 1 << 12)


def u64(rows):
    return np.array(rows, dtype=U64)


def run(ctx, trace, lookups):
    """the trace [columns][n] after one call"""
    trace = np.ascontiguousarray(trace, dtype=U64)
    d = ctx.alloc(trace.nbytes).upload(trace)
    try:
        ctx.lookup_columns(d.ptr, trace.shape[0], trace.shape[1], lookups)
        return d.download(trace.shape)
    finally:
        d.free()


@pytest.mark.parametrize("n", SIZES)
def test_every_case_equals_the_model_at_every_word(gpu, n):
    p, ctx = gpu
    for name in lc.CASES:
        inputs, table = lc.case(name, n)
        pin, ptab = lm.permuted_cols(inputs, table)
        got_in, got_table = p.permuted_cols(u64(inputs), u64(table), ctx=ctx)
        assert got_in.tolist() == pin, name
        assert got_table.tolist() == ptab, name


def test_the_arithmetic_tables_own_shape(gpu):
    # ArithmeticStark::generate_range_checks: the RANGE_COUNTER column 0 .. 65535 against a column of 16-bit limbs, n = 2^16
    p, ctx = gpu
    n = 1 << 16
    rng = np.random.Generator(np.random.PCG64(16))
    inputs, table = rng.integers(0, 1 << 16, size=n, dtype=U64), np.arange(n, dtype=U64)
    pin, ptab = lm.permuted_cols(inputs.tolist(), table.tolist())
    got_in, got_table = p.permuted_cols(inputs, table, ctx=ctx)
    assert got_in.tolist() == pin and got_table.tolist() == ptab
    assert all(lm.lookup_rows_vanish(pin, ptab))


# ------------------------------------------------------------------------------- calls of many lookups
def layout(count, n, kind, seed):
    """-> (trace [columns][n] with every output column filled with a marker, lookups, the model's outputs per lookup).  Columns are
    handed out in a seeded scattered order, with columns no lookup names in between."""
    rng = np.random.Generator(np.random.PCG64(seed))
    names = sorted(lc.CASES)
    sources = []                                                  # per lookup (inputs, table) as keys into `columns`
    columns = {}
    if kind == "shared-table":
        columns["t"] = [int(v) for v in rng.permutation(n)]
        for k in range(count):
            columns["a%d" % k] = [int(v) for v in rng.integers(0, n + (3 if k % 3 else 0), size=n)]      # two in three hold values not in the table
            sources.append(("a%d" % k, "t"))
    elif kind == "distinct-tables":
        for k in range(count):
            columns["a%d" % k], columns["t%d" % k] = lc.case(names[(5 * k + seed) % len(names)], n)
            sources.append(("a%d" % k, "t%d" % k))
    else:                                                         # "shared-input": lookups 2 k and 2 k + 1 look one input column up in two tables
        for k in range(count):
            if k % 2 == 0:
                columns["a%d" % k] = [int(v) for v in rng.integers(0, n, size=n)]
            columns["t%d" % k] = [int(v) for v in rng.integers(0, n, size=n)] if k % 2 else list(range(n))
            sources.append(("a%d" % (k - k % 2), "t%d" % k))
    keys = list(columns) + ["in%d" % k for k in range(count)] + ["out%d" % k for k in range(count)] + ["unused%d" % k for k in range(3)]
    place = {key: int(c) for key, c in zip(keys, rng.permutation(len(keys)))}
    trace = np.zeros((len(keys), n), dtype=U64)
    for key, c in place.items():
        trace[c] = u64(columns[key]) if key in columns else rng.integers(0, 2**64, size=n, dtype=U64)
    lookups = [(place[a], place[t], place["in%d" % k], place["out%d" % k]) for k, (a, t) in enumerate(sources)]
    cache, want = {}, []
    for a, t in sources:
        if (a, t) not in cache:
            cache[a, t] = lm.permuted_cols(columns[a], columns[t])
        want.append(cache[a, t])
    return trace, lookups, want


def check_call(ctx, trace, lookups, want, singles=True):
    got = run(ctx, trace, lookups)
    outputs = {c for lk in lookups for c in lk[2:]}
    for c in range(trace.shape[0]):
        if c not in outputs:
            assert (got[c] == trace[c]).all(), "column %d is no output and was changed" % c
    for lk, (pin, ptab) in zip(lookups, want):
        assert got[lk[2]].tolist() == pin and got[lk[3]].tolist() == ptab, lk
    assert (run(ctx, trace, lookups) == got).all(), "two identical calls give different words"
    if singles:
        for lk in lookups[:: max(1, len(lookups) // 5)]:
            alone = run(ctx, trace, [lk])
            assert (alone[lk[2]] == got[lk[2]]).all() and (alone[lk[3]] == got[lk[3]]).all(), lk
            others = [c for c in range(trace.shape[0]) if c not in lk[2:]]
            assert (alone[others] == trace[others]).all()


@pytest.mark.parametrize("kind", ["shared-table", "distinct-tables", "shared-input"])
@pytest.mark.parametrize("count", [1, 2, 33])
def test_calls_of_many_lookups(gpu, count, kind):
    p, ctx = gpu
    if kind == "shared-input" and count == 1:
        count = 4
    for n in (32, 1 << 11):
        trace, lookups, want = layout(count, n, kind, seed=count + n)
        check_call(ctx, trace, lookups, want)


def test_a_call_worked_in_two_chunks(gpu):
    # 130 lookups at n = 2^16 pass the 2^23 elements of a chunk: 128 lookups, then 2.  Two input columns in turn against one table, so that
    # the model runs twice; the shared table keeps its slot in the second chunk
    p, ctx = gpu
    n, count = 1 << 16, 130
    rng = np.random.Generator(np.random.PCG64(130))
    cols = [np.arange(n, dtype=U64), rng.integers(0, 1 << 16, size=n, dtype=U64), rng.integers(0, (1 << 16) + 2, size=n, dtype=U64)]
    want = [lm.permuted_cols(cols[k].tolist(), cols[0].tolist()) for k in (1, 2)]
    trace = np.zeros((3 + 2 * count, n), dtype=U64)
    trace[:3] = cols
    lookups = [(1 + k % 2, 0, 3 + 2 * k, 4 + 2 * k) for k in range(count)]
    got = run(ctx, trace, lookups)
    assert (got[:3] == trace[:3]).all()
    for k in range(count):
        pin, ptab = want[k % 2]
        assert (got[3 + 2 * k] == u64(pin)).all() and (got[4 + 2 * k] == u64(ptab)).all(), k


# ------------------------------------------------------------------------------- refusals
def test_every_refusal_and_the_trace_is_left_alone(gpu):
    p, ctx = gpu
    from plonky2_demo_amd import _lib
    n, columns = 32, 8
    rng = np.random.Generator(np.random.PCG64(3))
    trace = rng.integers(0, 2**64, size=(columns, n), dtype=U64)
    d = ctx.alloc(trace.nbytes).upload(trace)

    def status(lookups, n=n, columns=columns, ptr=d.ptr, handle=ctx.handle, count=None, null_lookups=False):
        flat = np.ascontiguousarray(lookups, dtype=np.uint32).reshape(-1, 4)
        arg = None if null_lookups else flat.ctypes.data_as(ctypes.c_void_p)
        return _lib.lib.gl_stark_lookup_columns(handle, ptr, columns, n, arg, flat.shape[0] if count is None else count)
    try:
        ok = [(0, 1, 2, 3)]
        assert status(ok, handle=None) == GL_ERR_ARG and status(ok, ptr=None) == GL_ERR_ARG and status(ok, null_lookups=True) == GL_ERR_ARG
        assert status(ok, count=0) == GL_ERR_ARG
        many = [(0, 1, 2, 3)] * 1025
        assert status(many) == GL_ERR_ARG                           # count > 1024 (refused before anything else is looked at)
        for bad_n in (0, 1, 3, 24, 48, (1 << 24) + 1, 1 << 25):
            assert status(ok, n=bad_n) == GL_ERR_ARG, bad_n
        for field in range(4):
            for bad in (columns, columns + 1, 2**32 - 1):
                lk = list(ok[0])
                lk[field] = bad
                assert status([lk]) == GL_ERR_ARG, (field, bad)
        refused = [
            [(0, 1, 0, 3)], [(0, 1, 1, 3)], [(0, 1, 2, 0)], [(0, 1, 2, 1)],      # an output that is the lookup's own input or table
            [(0, 1, 2, 2)],                                                     # its two outputs on one column
            [(0, 1, 2, 3), (4, 5, 6, 3)], [(0, 1, 2, 3), (4, 5, 2, 6)], [(0, 1, 2, 3), (4, 5, 3, 6)],      # two lookups share an output
            [(0, 1, 2, 3), (4, 5, 6, 0)], [(0, 1, 2, 3), (4, 5, 1, 6)],          # an output that is another lookup's input or table
            [(0, 1, 4, 3), (4, 5, 6, 7)], [(0, 1, 2, 5), (4, 5, 6, 7)],          # ... of a LATER lookup
        ]
        for lookups in refused:
            assert status(lookups) == GL_ERR_ARG, lookups
            assert "gl_stark_lookup_columns" in (_lib.lib.gl_last_error() or b"").decode()
        assert (d.download(trace.shape) == trace).all(), "a refused call changed the trace"
        # what is allowed: shared inputs and shared tables
        assert status([(0, 1, 2, 3), (0, 1, 4, 5), (0, 6, 7, 3 + 0)][:2]) == 0
        assert status([(0, 1, 2, 3), (1, 0, 4, 5)]) == 0             # one column an input here and a table there
    finally:
        d.free()


# ------------------------------------------------------------------------------- end to end: a range-checked table from a device trace
def prove_from_the_device(p, ctx, stark, value, counter):
    n = len(value)
    trace = np.zeros((4, n), dtype=U64)
    trace[lc.VALUE], trace[lc.COUNTER] = u64(value), u64(counter)
    d = ctx.alloc(trace.nbytes).upload(trace)
    try:
        ctx.lookup_columns(d.ptr, 4, n, [(lc.VALUE, lc.COUNTER, lc.PERMUTED_VALUE, lc.PERMUTED_COUNTER)])
        return stark.prove_device(d.ptr, [])
    finally:
        d.free()


@pytest.mark.parametrize("lg_n,r", [(5, 20), (12, 4096)])
def test_a_range_checked_table_proved_without_the_trace_leaving_the_device(gpu, orc, lg_n, r):
    from test_fri_openings import model_challenger, verify_path_of
    p, ctx = gpu
    n, nc = 1 << lg_n, 2
    air = lc.range_check_air(p.lookup_constraints, r)
    assert (air.constraint_degree, air.q) == (3, 2)
    config = p.StarkConfig.standard_fast_config()
    assert config.num_challenges == nc
    stark = p.Stark(p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs), config, lg_n, ctx=ctx)
    value, counter = lc.range_check_columns(n, r)
    queries = 8 if lg_n == 12 else None

    def model_verdict(proof):
        return sm.verify(air, nc, stark.params, proof, model_challenger(orc, "poseidon"), verify_path_of(orc, "poseidon"), max_queries=queries)
    proof = prove_from_the_device(p, ctx, stark, value, counter)
    assert stark.verify(proof) == (True, "", 0)
    assert model_verdict(proof) == sm.fom.ACCEPTED
    pin, ptab = lm.permuted_cols(value, counter)
    assert proof == stark.prove(u64([value, counter, pin, ptab]), [])
    # one value out of range: q = 2 is a power of two, so the prover's trim has nothing to look at; the identity at zeta fails
    value[n // 3] = r
    bad = prove_from_the_device(p, ctx, stark, value, counter)
    ok, why, code = stark.verify(bad)
    assert (ok, code) == (False, sm.VANISHING) and "anishing" in why
    assert model_verdict(bad) == sm.VANISHING
