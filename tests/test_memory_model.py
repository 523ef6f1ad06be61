"""CPU tests of the memory table (evm/src/memory): the sequential model of tests/memory_model.py against logs worked by hand,
gl_memory_trace_host against the model at every word of every crafted log of tests/memory_cases.py and of random ones, the description
gl_memory_stark_desc exports against the model's eval_packed_generic (values, order, and every constraint violated by a corruption of
its own), gl_stark_check, the host refusals, the committed GPU-made proof, and the compiler's resource report of the device unit.
No GPU."""
import ctypes
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import memory_cases as mc
import memory_model as mm
import stark_model as sm
from memory_model import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL_ERR_ARG, GL_ERR_UNSUPPORTED = 1, 3
FILTERS = {"all": 0, "transition": 1, "first_row": 2, "last_row": 3}


def column(trace, c):
    return [int(v) for v in trace[c]]


# ------------------------------------------------------------------------------- the model, pinned by hand
def test_the_model_on_the_doc_comments_timestamps_20_and_100():
    # 32 ops: max_rc = 31.  The address accessed at 20 and 100: 100 - 20 = 80 > 31 pushes a read at 51; 100 - 51 = 49 > 31 pushes one at
    # 82; 100 - 82 = 18 ends the loop (the comment's "say 50 and 80").  34 rows pad to 64 with copies of the LAST PUSHED row, the read at
    # 82, which the second sort leaves directly behind it: rows 0..32 are 20, 51, 82 and thirty copies of 82, then 100.
    trace = mm.generate_trace(mc.CASES["timestamps-20-and-100"])
    assert len(trace[0]) == 64
    assert column(trace, mm.ADDR_VIRTUAL)[:34] == [1] * 34 and column(trace, mm.ADDR_VIRTUAL)[34:] == list(range(2, 32))
    assert column(trace, mm.TIMESTAMP)[:34] == [20, 51] + [82] * 31 + [100]
    assert column(trace, mm.FILTER)[:34] == [1] + [0] * 32 + [1] and column(trace, mm.IS_READ)[:34] == [0] + [1] * 33
    assert column(trace, mm.RANGE_CHECK)[:34] == [31, 31] + [0] * 30 + [18, 0]      # the last: virt 1 -> 2, a step of one, minus one
    assert column(trace, mm.VIRTUAL_FIRST_CHANGE)[:34] == [0] * 33 + [1]
    limbs = mc.CASES["timestamps-20-and-100"][0]["value"]
    assert all(column(trace, mm.value_limb(j))[:34] == [limbs[j]] * 34 for j in range(8))      # the pushed reads carry curr.value
    assert column(trace, mm.COUNTER) == list(range(64)) and column(trace, mm.RANGE_CHECK_PERMUTED) == sorted(column(trace, mm.RANGE_CHECK))


def test_the_model_on_a_virt_gap_worked_by_hand():
    # four ops: max_rc = 3.  virt 0 -> 5: 5 - 0 - 1 = 4 > 3 pushes a read of ZERO at virt 4 with timestamp 0; 5 - 4 - 1 = 0 ends the loop.
    # Five rows pad to eight with three copies of the pushed row behind it (rows 1..4), in the middle of the trace.
    trace = mm.generate_trace(mc.CASES["virt-gap-of-max-rc-plus-one"])
    assert column(trace, mm.ADDR_VIRTUAL) == [0, 4, 4, 4, 4, 5, 6, 7]
    assert column(trace, mm.TIMESTAMP) == [1, 0, 0, 0, 0, 2, 3, 4]
    assert column(trace, mm.FILTER) == [1, 0, 0, 0, 0, 1, 1, 1] and column(trace, mm.IS_READ) == [0, 1, 1, 1, 1, 0, 0, 0]
    assert column(trace, mm.value_limb(0)) == [1, 0, 0, 0, 0, 2, 3, 4]
    assert column(trace, mm.VIRTUAL_FIRST_CHANGE) == [1, 0, 0, 0, 1, 1, 1, 0]
    assert column(trace, mm.RANGE_CHECK) == [3, 0, 0, 0, 0, 0, 0, 0]
    # ... and a gap of exactly max_rc pushes nothing
    assert column(mm.generate_trace(mc.CASES["virt-gap-of-max-rc"]), mm.ADDR_VIRTUAL) == [0, 4, 5, 6]
    assert column(mm.generate_trace(mc.CASES["virt-gap-of-max-rc"]), mm.RANGE_CHECK) == [3, 0, 0, 0]


def test_the_model_on_a_tie_worked_by_hand():
    # three ops, two of them with one key: the stable sort keeps their issue order, nothing is pushed, and the padding row copies the LAST
    # of the tie (value 3) as a read with filter 0
    trace = mm.generate_trace(mc.CASES["no-dummies-padding-behind-a-tie"])
    assert column(trace, mm.value_limb(0)) == [1, 2, 3, 3] and column(trace, mm.FILTER) == [1, 1, 1, 0] and column(trace, mm.IS_READ) == [0, 0, 0, 1]
    assert column(trace, mm.RANGE_CHECK) == [0, 0, 0, 0] and column(trace, mm.VIRTUAL_FIRST_CHANGE) == [1, 0, 0, 0]
    # timestamps: a step of max_rc pushes nothing, max_rc + 1 one row
    assert column(mm.generate_trace(mc.CASES["timestamp-gap-of-max-rc"]), mm.TIMESTAMP) == [1, 4, 5, 6]
    assert column(mm.generate_trace(mc.CASES["timestamp-gap-of-max-rc-plus-one"]), mm.TIMESTAMP) == [1, 4, 4, 4, 4, 5, 6, 7]


def test_the_model_raises_the_references_assertion():
    for name, log in mc.REFUSED.items():
        with pytest.raises(mm.RangeCheckTooLarge):
            mm.generate_trace(log)
    for name, log in mc.ALLOWED_STEPS.items():
        mm.generate_trace(log)


# ------------------------------------------------------------------------------- the host entry
@pytest.fixture(scope="module")
def modelled():
    """name -> the model's trace as [26][n] uint64, computed once and left unchanged"""
    return {name: np.array(mm.generate_trace(log), dtype=np.uint64) for name, log in mc.CASES.items()}


def test_the_crafted_logs_cover_what_they_are_named_for(modelled):
    heights = {name: t.shape[1] for name, t in modelled.items()}
    assert heights["one-op"] == 1 and heights["two-ops"] == 2 and heights["three-ops"] == 4
    assert heights["gap-rows-push-the-height-over-a-power-of-two"] == 16 and heights["one-pair-asks-for-5000-rows"] == 1 << 13
    assert heights["one-virt-pair-asks-for-5000-rows"] == 1 << 13 and max(heights.values()) == 1 << 13
    t = modelled["dummies-from-several-pairs-padding-mid-trace"]
    padding = [i for i in range(1, t.shape[1]) if (t[:14, i] == t[:14, i - 1]).all() and t[mm.FILTER, i] == 0]
    assert padding and padding[-1] < t.shape[1] - 2, "the padding block does not stand mid-trace"
    t = modelled["first-change-in-each-part"]
    assert t[mm.CONTEXT_FIRST_CHANGE].any() and t[mm.SEGMENT_FIRST_CHANGE].any() and t[mm.VIRTUAL_FIRST_CHANGE].any()


def test_the_host_entry_equals_the_model_at_every_word_of_every_case(modelled):
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    for name, log in mc.CASES.items():
        ops = mc.records(log)
        got = p.memory_trace_host(ops)
        assert got.shape == modelled[name].shape, name
        assert (got == modelled[name]).all(), name
        n = ctypes.c_size_t()
        assert _lib.lib.gl_memory_trace_host(ops.ctypes.data_as(ctypes.c_void_p), ops.size, None, 0, ctypes.byref(n)) == 0      # cols_out == NULL reports n alone
        assert n.value == modelled[name].shape[1], name


def random_ops(rng, num_ops):
    """any log, consistent or not: few addresses far apart, timestamps with ties and large steps"""
    contexts, segments = [0, 1, 2][: int(rng.integers(1, 4))], [0, 1][: int(rng.integers(1, 3))]
    virts = [int(v) for v in rng.integers(0, int(rng.choice([4, 64, 3000])), size=int(rng.integers(1, 6)))]
    top = int(rng.choice([4, 40, 2500]))
    return [mm.op(int(rng.choice(contexts)), int(rng.choice(segments)), int(rng.choice(virts)), int(rng.integers(0, top)), int(rng.integers(0, 1 << 62)) << 190 | int(rng.integers(0, 9)),
                  is_read=int(rng.integers(0, 2)), filter=int(rng.integers(0, 2))) for _ in range(num_ops)]


def test_the_host_entry_equals_the_model_on_random_logs():
    import plonky2_demo_amd as p
    rng = np.random.Generator(np.random.PCG64(20))
    pushed = 0
    for k in range(150):
        log = random_ops(rng, int(rng.integers(1, 40)))
        want = np.array(mm.generate_trace(log), dtype=np.uint64)
        assert (p.memory_trace_host(mc.records(log)) == want).all(), k
        pushed += want.shape[1] > mm.next_power_of_two(len(log))
    assert pushed >= 30                                                  # gap rows that push the height over the next power of two, often


def test_every_host_refusal_leaves_the_output_untouched():
    from plonky2_demo_amd import _lib
    marker = 0xA5A5A5A5A5A5A5A5
    out = np.full((26, 16), marker, dtype=np.uint64)
    n = ctypes.c_size_t(0)

    def status(ops, num_ops=None, cols=out, capacity=16, n_ptr=True):
        return _lib.lib.gl_memory_trace_host(ops.ctypes.data_as(ctypes.c_void_p) if ops is not None else None, ops.size if num_ops is None else num_ops,
                                             cols.ctypes.data_as(ctypes.c_void_p) if cols is not None else None, capacity, ctypes.byref(n) if n_ptr else None)
    good = mc.records(mc.CASES["three-ops"])
    assert status(None, num_ops=3) == GL_ERR_ARG and status(good, n_ptr=False) == GL_ERR_ARG
    assert status(good, num_ops=0) == GL_ERR_ARG
    for field in ("filter", "is_read"):
        for bad in (2, 0xFFFFFFFF):
            ops = good.copy()
            ops[field][1] = bad
            assert status(ops) == GL_ERR_ARG, (field, bad)
    for name, log in mc.REFUSED.items():
        assert status(mc.records(log)) == GL_ERR_ARG, name
        assert status(mc.records(log), cols=None) == GL_ERR_ARG, name
    for name, log in mc.TOO_HIGH.items():
        assert status(mc.records(log)) == GL_ERR_UNSUPPORTED, name
        assert status(mc.records(log), cols=None) == GL_ERR_UNSUPPORTED, name
    assert status(good, capacity=3) == GL_ERR_ARG                        # capacity_rows < n = 4
    assert (out == marker).all(), "a refused call wrote to the output"
    for name, log in mc.ALLOWED_STEPS.items():
        assert status(mc.records(log)) == 0, name
    assert status(good, capacity=4) == 0 and n.value == 4


# ------------------------------------------------------------------------------- the description
@pytest.fixture(scope="module")
def desc():
    import plonky2_demo_amd as p
    return p.memory_stark()


def as_air(desc):
    return SimpleNamespace(constraints=desc.constraints, pairs=desc.pairs, q=desc.quotient_degree_factor, num_columns=desc.num_columns)


def test_the_description_is_memory_starks_shape(desc):
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree) == (26, 0, 3)
    assert len(desc.constraints) == 21 + 2 and desc.pairs == [[(22, 24)], [(23, 25)]]
    assert desc.constraints[21:] == [(f, [(c, list(ops)) for c, ops in terms]) for f, terms in p.lookup_constraints(24, 25)]
    assert max(len(ops) for _, terms in desc.constraints for _, ops in terms) == 3
    for name in ("NUM_CHANNELS", "FILTER", "TIMESTAMP", "IS_READ", "ADDR_CONTEXT", "ADDR_SEGMENT", "ADDR_VIRTUAL", "CONTEXT_FIRST_CHANGE", "SEGMENT_FIRST_CHANGE",
                 "VIRTUAL_FIRST_CHANGE", "RANGE_CHECK", "COUNTER", "RANGE_CHECK_PERMUTED", "COUNTER_PERMUTED", "NUM_COLUMNS"):
        assert getattr(_lib, "GL_MEMORY_" + name) == getattr(mm, name), name
    assert _lib.GL_MEMORY_VALUE_START == mm.value_limb(0) and p.MEMORY_OP_DTYPE.itemsize == 56
    header = open(os.path.join(ROOT, "include", "plonky2_mi355x.h")).read()
    for name in ("FILTER", "TIMESTAMP", "IS_READ", "ADDR_CONTEXT", "ADDR_SEGMENT", "ADDR_VIRTUAL", "VALUE_START", "CONTEXT_FIRST_CHANGE", "SEGMENT_FIRST_CHANGE",
                 "VIRTUAL_FIRST_CHANGE", "RANGE_CHECK", "COUNTER", "RANGE_CHECK_PERMUTED", "COUNTER_PERMUTED", "NUM_COLUMNS", "NUM_CHANNELS"):
        assert int(re.search(r"#define GL_MEMORY_%s (\d+)u" % name, header).group(1)) == getattr(_lib, "GL_MEMORY_" + name), name
    # ctl_data / ctl_filter (memory_stark.rs:30-40)
    assert [c.flat() for c in p.memory_ctl_data()] == [([(c, 1)], 0) for c in [2, 3, 4, 5] + list(range(6, 14)) + [1]]
    assert p.memory_ctl_filter().flat() == ([(0, 1)], 0)


@pytest.mark.parametrize("lg_n", [4, 5, 13, 20])
def test_gl_stark_check_accepts_the_description(desc, lg_n):
    import plonky2_demo_amd as p
    desc.check(p.StarkConfig.standard_fast_config(), lg_n)


def test_the_descriptions_constraints_are_eval_packed_generic_one_by_one(desc):
    air = as_air(desc)
    assert [f for f, _ in desc.constraints] == [FILTERS[f] for f, _ in mm.eval_packed_generic(sm.Base, [0] * 26, [0] * 26)]
    rng = np.random.Generator(np.random.PCG64(26))
    for k in range(200):                                                 # random, invalid row pairs: nothing vanishes by accident
        local = [int(v) for v in rng.integers(0, P, size=26, dtype=np.uint64)]
        nxt = [int(v) for v in rng.integers(0, P, size=26, dtype=np.uint64)]
        want = [v for _, v in mm.eval_packed_generic(sm.Base, local, nxt)]
        assert sm.constraint_values(sm.Base, air, local, nxt, []) == want, k
        assert all(want)
        if k < 40:
            el, en = [(v, int(w)) for v, w in zip(local, rng.integers(0, P, size=26, dtype=np.uint64))], [(v, int(w)) for v, w in zip(nxt, rng.integers(0, P, size=26, dtype=np.uint64))]
            assert sm.constraint_values(sm.Ext, air, el, en, []) == [v for _, v in mm.eval_packed_generic(sm.Ext, el, en)], k


def violated(air, trace):
    """the constraints that do not vanish somewhere on the trace, each under its filter"""
    n, out = len(trace[0]), set()
    rows = [[int(col[i]) for col in trace] for i in range(n)]
    for i in range(n):
        for c, ((filt, _), v) in enumerate(zip(air.constraints, sm.constraint_values(sm.Base, air, rows[i], rows[(i + 1) % n], []))):
            on = {0: True, 1: i != n - 1, 2: i == 0, 3: i == n - 1}[filt]
            if on and v:
                out.add(c)
    return out


def test_the_constraints_hold_on_every_model_trace(desc, modelled):
    air = as_air(desc)
    for name, trace in modelled.items():
        assert violated(air, trace.tolist()) == set(), name
    assert violated(air, mm.generate_trace(mc.mismatched_read())) == {13}      # the read's limb 0 differs from the write's


def test_every_constraint_is_violated_by_a_corruption_of_its_own(desc, modelled):
    air = as_air(desc)
    base = modelled["dummies-from-several-pairs-padding-mid-trace"].tolist()
    n = len(base[0])
    assert violated(air, base) == set()

    def row_where(pred):
        return next(i for i in range(n - 1) if pred(i))
    cfc, sfc, vfc = (lambda i: base[mm.CONTEXT_FIRST_CHANGE][i] == 1), (lambda i: base[mm.SEGMENT_FIRST_CHANGE][i] == 1), (lambda i: base[mm.VIRTUAL_FIRST_CHANGE][i] == 1)
    quiet = row_where(lambda i: not (cfc(i) or sfc(i) or vfc(i)))
    read_next = row_where(lambda i: not (cfc(i) or sfc(i) or vfc(i)) and base[mm.IS_READ][i + 1] == 1)       # the next row reads this row's address
    pin, ptab = base[mm.RANGE_CHECK_PERMUTED], base[mm.COUNTER_PERMUTED]
    step = next(i for i in range(1, n) if pin[i] != pin[i - 1])
    # constraint -> (row, column, new word): one word of a valid trace changed
    corruptions = {
        0: (quiet, mm.FILTER, 2),
        1: (row_where(lambda i: base[mm.FILTER][i] == 0), mm.IS_READ, 0),
        2: (quiet, mm.CONTEXT_FIRST_CHANGE, 2),
        3: (quiet, mm.SEGMENT_FIRST_CHANGE, 2),
        4: (quiet, mm.VIRTUAL_FIRST_CHANGE, 2),
        5: (row_where(sfc), mm.CONTEXT_FIRST_CHANGE, 1),
        6: (row_where(cfc), mm.SEGMENT_FIRST_CHANGE, 1),
        7: (row_where(cfc), mm.VIRTUAL_FIRST_CHANGE, 1),
        8: (row_where(sfc), mm.VIRTUAL_FIRST_CHANGE, 1),
        9: (row_where(cfc), mm.CONTEXT_FIRST_CHANGE, 0),
        10: (row_where(sfc), mm.SEGMENT_FIRST_CHANGE, 0),
        11: (row_where(vfc), mm.VIRTUAL_FIRST_CHANGE, 0),
        12: (quiet, mm.RANGE_CHECK, base[mm.RANGE_CHECK][quiet] + 1),
        21: (step, mm.COUNTER_PERMUTED, (ptab[step] + 1) % P),
        22: (0, mm.COUNTER_PERMUTED, (ptab[0] + 1) % P),
    }
    for limb in range(8):
        corruptions[13 + limb] = (read_next, mm.value_limb(limb), base[mm.value_limb(limb)][read_next] + 1)
    assert sorted(corruptions) == list(range(23)), "a constraint goes unexercised"
    assert len(set(corruptions.values())) == 23, "two constraints share a corruption"
    for c, (row, col, word) in sorted(corruptions.items()):
        trace = [list(column) for column in base]
        assert trace[col][row] != word
        trace[col][row] = word
        assert c in violated(air, trace), (c, row, col, word)


# ------------------------------------------------------------------------------- the committed GPU-made proof
def test_the_committed_proof_verifies_and_a_flipped_byte_does_not(desc):
    import plonky2_demo_amd as p
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "memory_stark_n32.json")) as f:
        meta = json.load(f)
    proof = open(os.path.join(golden, "memory_stark_n32.bin"), "rb").read()
    ops = np.array([tuple(o[:6]) + (o[6],) for o in meta["ops"]], dtype=p.MEMORY_OP_DTYPE)
    assert meta["num_rows"] == 32 and p.memory_trace_host(ops).shape == (26, 32) and len(proof) == meta["num_bytes"]
    config = p.StarkConfig.standard_fast_config()
    assert p.stark_verify(desc, config, 5, proof) == (True, "", 0)
    for pos in (0, len(proof) // 2, len(proof) - 1):
        bad = bytearray(proof)
        bad[pos] ^= 1
        assert p.stark_verify(desc, config, 5, bytes(bad))[0] is False, pos


# ------------------------------------------------------------------------------- the device unit's resource report
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


def test_every_memory_trace_kernel_compiles_without_scratch_and_the_committed_report_is_current():
    # no runtime-indexed private arrays: the compiler is asked (device code only, no GPU), and profiles/memory_trace_resource_usage.txt
    # must be what it answers for the k_* kernels: the k_* entries of `make -s -C plonky2_demo_amd/csrc memory_trace.resource_usage`
    report = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "plonky2_demo_amd", "csrc"), "memory_trace.resource_usage"], capture_output=True, text=True,
                            timeout=600)
    assert report.returncode == 0, report.stderr
    fresh = _kernel_blocks(report.stdout)
    names = [ln for ln in fresh if "Function Name:" in ln]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", "\n".join(fresh))]
    with open(os.path.join(ROOT, "plonky2_demo_amd", "csrc", "memory_trace_kernels.cuh")) as f:
        declared = re.findall(r"__global__[^\n]*?void (k_\w+)", f.read())
    own = [ln for ln in names if "k_mem_" in ln]
    assert len(set(declared)) == 9 and len(own) == 9 and len(names) == len(scratch) and not any(scratch), "\n".join(fresh)
    assert all(any(k in ln for ln in names) for k in declared)
    with open(os.path.join(ROOT, "profiles", "memory_trace_resource_usage.txt")) as f:
        committed = _kernel_blocks(f.read())
    assert committed == fresh, "profiles/memory_trace_resource_usage.txt is stale"
