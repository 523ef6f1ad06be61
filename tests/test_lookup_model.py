"""CPU tests of the lookup columns (evm/src/lookup.rs): the sequential model of tests/lookup_model.py against examples worked by hand,
gl_permuted_cols_host against the model on every crafted case, the properties that make the columns a lookup argument,
lookup_constraints against eval_lookups, gl_stark_check on the range-check AIR, and the compiler's resource report of the device unit.
No GPU."""
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import lookup_cases as lc
import lookup_model as lm
import stark_model as sm
from lookup_model import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 32, 256)


def test_the_model_on_a_lifo_pop_worked_by_hand():
    # sorted inputs 2 2 2 3, sorted table 0 1 2 3.
    #   2 > 0: push 0.  2 > 1: push 1.  2 = 2: permuted_table[0] = 2.
    #   2 < 3: pop 1 -> permuted_table[1] = 1.  2 < 3: pop 0 -> permuted_table[2] = 0 (last in, first out).
    #   3 = 3: permuted_table[3] = 3.  Nothing is left over.
    assert lm.permuted_cols([3, 2, 2, 2], [2, 0, 3, 1]) == ([2, 2, 2, 3], [2, 1, 0, 3])


def test_the_model_on_a_deferred_fill_worked_by_hand():
    # sorted inputs 0 0 0 3, sorted table 0 1 2 3.
    #   0 = 0: permuted_table[0] = 0.  0 < 1 on an empty stack: position 1 deferred.  0 < 1 again: position 2 deferred.
    #   3 > 1: push 1.  3 > 2: push 2.  3 = 3: permuted_table[3] = 3; the inputs are used up.
    #   The deferred positions 1, 2 take the stack from the BOTTOM: 1, 2.
    assert lm.permuted_cols([0, 3, 0, 0], [3, 2, 1, 0]) == ([0, 0, 0, 3], [0, 1, 2, 3])


def test_the_model_when_the_loop_leaves_at_the_end_of_the_table_with_a_full_stack_worked_by_hand():
    # sorted inputs 1 5 5 5, sorted table 0 1 2 3.
    #   1 > 0: push 0.  1 = 1: permuted_table[0] = 1.  5 > 2: push 2.  5 > 3: push 3.  j == n: the loop leaves with the stack 0 2 3.
    #   The inputs at positions 1, 2, 3 never pop: they take the stack from the bottom, 0 2 3 -- not 3 2 0.
    assert lm.permuted_cols([5, 1, 5, 5], [0, 1, 2, 3]) == ([1, 5, 5, 5], [1, 0, 2, 3])
    # ... and non-canonical words are compared by their canonical values: p + 1 is 1
    assert lm.permuted_cols([5, P + 1, 5, 5], [P, 1, 2, 3]) == ([1, 5, 5, 5], [1, 0, 2, 3])


@pytest.fixture(scope="module")
def modelled():
    """(name, n) -> (inputs, table, permuted inputs, permuted table) of the model, computed once"""
    out = {}
    for n in SIZES:
        for name in lc.CASES:
            inputs, table = lc.case(name, n)
            out[name, n] = (inputs, table) + lm.permuted_cols(inputs, table)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_the_host_entry_equals_the_model_on_every_case(modelled, n):
    import plonky2_demo_amd as p
    for name in lc.CASES:
        inputs, table, pin, ptab = modelled[name, n]
        got_in, got_table = p.permuted_cols_host(np.array(inputs, dtype=np.uint64), np.array(table, dtype=np.uint64))
        assert got_in.tolist() == pin, name
        assert got_table.tolist() == ptab, name


def test_the_host_entry_refuses_nulls_and_an_empty_column():
    import ctypes
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    a = np.zeros(4, dtype=np.uint64)
    ptr = a.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, ptr, 4, ptr, ptr), (ptr, None, 4, ptr, ptr), (ptr, ptr, 4, None, ptr), (ptr, ptr, 4, ptr, None), (ptr, ptr, 0, ptr, ptr)):
        assert _lib.lib.gl_permuted_cols_host(*args) == 1        # GL_ERR_ARG
    with pytest.raises(ValueError):
        p.permuted_cols_host([1, 2], [1])


@pytest.mark.parametrize("n", SIZES)
def test_the_columns_are_a_lookup_argument_exactly_when_the_lookup_is_valid(modelled, n):
    seen_valid = seen_invalid = 0
    for name in lc.CASES:
        inputs, table, pin, ptab = modelled[name, n]
        assert pin == sorted(int(x) % P for x in inputs), name
        assert sorted(ptab) == sorted(int(x) % P for x in table), name
        rows = lm.lookup_rows_vanish(pin, ptab)
        if lc.is_valid(inputs, table):
            assert all(rows), name                                # both constraints on all n rows, the wrap row among them
            seen_valid += 1
        else:
            assert not all(rows), name
            seen_invalid += 1
        if name in lc.INVALID:
            assert not lc.is_valid(inputs, table), name
    assert seen_invalid >= len(lc.INVALID) and seen_valid >= (6 if n == 1 else len(lc.CASES) - len(lc.INVALID) - 4)


def test_lookup_constraints_are_eval_lookups_through_the_consumer():
    import plonky2_demo_amd as p
    from stark_airs import ALL, LAST_ROW
    rng = np.random.Generator(np.random.PCG64(5))
    for col_in, col_table, width in ((2, 3, 4), (0, 1, 2), (7, 5, 9), (4, 4, 5)):
        constraints = p.lookup_constraints(col_in, col_table)
        assert [f for f, _ in constraints] == [ALL, LAST_ROW] and [len(t) for _, t in constraints] == [4, 2]
        air = SimpleNamespace(constraints=constraints, pairs=[], q=2)
        for k in range(50):
            local = [int(v) for v in rng.integers(0, P, size=width, dtype=np.uint64)]
            nxt = [int(v) for v in rng.integers(0, P, size=width, dtype=np.uint64)]
            if k % 5 == 0:
                nxt[col_in] = local[col_in]                       # the vertical difference vanishes
            if k % 7 == 0:
                nxt[col_table] = nxt[col_in]                      # the horizontal one does
            want = lm.eval_lookups(local[col_in], nxt[col_in], nxt[col_table])
            assert tuple(sm.constraint_values(sm.Base, air, local, nxt, [])) == want
            ext = sm.constraint_values(sm.Ext, air, [(v, 0) for v in local], [(v, 0) for v in nxt], [])
            assert tuple(ext) == ((want[0], 0), (want[1], 0))
            # through the consumer: alpha-weighted, the second under L_last
            z_last, l_first, l_last, alpha = (int(v) for v in rng.integers(0, P, size=4, dtype=np.uint64))
            acc, = sm.eval_vanishing(sm.Base, air, 1, local, nxt, [], [alpha], z_last, l_first, l_last)
            assert acc == (want[0] * alpha + want[1] * l_last) % P


@pytest.mark.parametrize("r,lg_n", [(1, 5), (7, 5), (32, 5), (4096, 12)])
def test_the_range_check_air_passes_gl_stark_check_and_its_trace_satisfies_it(r, lg_n):
    import plonky2_demo_amd as p
    from stark_airs import ALL, FIRST_ROW, LAST_ROW, TRANSITION
    air = lc.range_check_air(p.lookup_constraints, r)
    desc = p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs)
    desc.check(p.StarkConfig.standard_fast_config(), lg_n)
    if lg_n > 5:
        return
    n = 1 << lg_n
    value, counter = lc.range_check_columns(n, r)
    pin, ptab = lm.permuted_cols(value, counter)
    cols = [value, counter, pin, ptab]
    for i in range(n):
        local, nxt = [c[i] for c in cols], [c[(i + 1) % n] for c in cols]
        for (filt, _), v in zip(air.constraints, sm.constraint_values(sm.Base, air, local, nxt, [])):
            on = {ALL: True, TRANSITION: i != n - 1, FIRST_ROW: i == 0, LAST_ROW: i == n - 1}[filt]
            assert v == 0 or not on, (i, filt)
    for a, b in ((0, 2), (1, 3)):
        assert sorted(cols[a]) == sorted(cols[b])


def _kernel_blocks(report):
    """the report's lines of the project's own kernels (k_*), source positions left out: the library's sort kernels stand in the same report"""
    lines = [re.sub(r"^\S+?:\d+:\d+: ", "", ln) for ln in report.splitlines()]
    out, keep = [], False
    for ln in lines:
        if "Function Name:" in ln:
            keep = re.search(r"Function Name: _Z\d+k_\w+", ln) is not None
        if keep:
            out.append(ln)
    return out


def test_every_lookup_kernel_compiles_without_scratch_and_the_committed_report_is_current():
    # no runtime-indexed private arrays: the compiler is asked (device code only, no GPU), and profiles/stark_lookup_resource_usage.txt
    # must be what it answers for the k_* kernels: the k_* entries of `make -s -C plonky2_demo_amd/csrc stark_lookup.resource_usage`
    report = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "plonky2_demo_amd", "csrc"), "stark_lookup.resource_usage"], capture_output=True, text=True,
                            timeout=600)
    assert report.returncode == 0, report.stderr
    fresh = _kernel_blocks(report.stdout)
    names = [ln for ln in fresh if "Function Name:" in ln]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", "\n".join(fresh))]
    with open(os.path.join(ROOT, "plonky2_demo_amd", "csrc", "stark_lookup_kernels.cuh")) as f:
        declared = re.findall(r"__global__[^\n]*?void (k_\w+)", f.read())
    assert len(set(declared)) == 9 and len(names) == len(scratch) == 9 and not any(scratch), "\n".join(fresh)
    assert all(any(k in ln for ln in names) for k in declared)
    with open(os.path.join(ROOT, "profiles", "stark_lookup_resource_usage.txt")) as f:
        committed = _kernel_blocks(f.read())
    assert committed == fresh, "profiles/stark_lookup_resource_usage.txt is stale"
