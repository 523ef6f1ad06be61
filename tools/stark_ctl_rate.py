#!/usr/bin/env python3
"""Device time of the cross-table-lookup phases of a table set against the trace commitment (run on the GPU).

    python tools/stark_ctl_rate.py [--rows-log 16 18 20] [--out FILE]

A set of three 32-column degree-3 tables under StarkConfig::standard_fast_config (num_challenges 2): tables 0 and 1 look three columns
up in table 2 under filter columns, and table 2 looks four unfiltered Columns (one an le_bits combination of 8 columns, one with a
constant) up in table 0: 4 CTL Zs on tables 0 and 2, 2 on table 1.  The traces are random with binary filter columns; they need not
be consistent, since only the phases are timed.  Per table size, summed over the three tables, the median device time (HIP events on
the context's stream, gl_ctx_timing_*) of
  - the trace commitments (IFFT, LDE, Merkle),
  - the CTL Z phase: the factor kernel and the three launches of the inclusive scan,
  - the single-table quotient launch and the CTL pass that follows it,
  - the whole set proof (gl_stark_set_prove): the sum of every timed device scope of one proof, and its wall time from host traces.
Prints a markdown table (profiles/README.md holds the one from the one run made).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonky2_demo_amd as p  # noqa: E402

P = p.GOLDILOCKS_ORDER
COLUMNS, NC = 32, 2


def system(lg_n, config):
    C, T = p.CtlColumn, p.TableWithColumns
    desc = p.StarkDesc(COLUMNS, 0, 3, [(p.GL_STARK_ALL, [(1, [(p.GL_STARK_LOCAL, 3), (p.GL_STARK_LOCAL, 3)]), (P - 1, [(p.GL_STARK_LOCAL, 3)])])])
    lookups = [
        p.CrossTableLookup([T(0, C.singles([0, 1, 2]), C.single(3)), T(1, C.singles([0, 1, 2]), C.sum([3, 4]))], T(2, C.singles([0, 1, 2]), C.single(3))),
        p.CrossTableLookup([T(2, [C.le_bits(range(8, 16)), C.linear_combination([(16, 3)], 7), C.single(17), C.single(18)])], T(0, C.singles([5, 6, 7, 8]))),
    ]
    return p.StarkSetDesc([(desc, lg_n)] * 3, lookups, config)


def trace_of(rng, n):
    t = rng.integers(0, P, size=(COLUMNS, n), dtype=np.uint64)
    t[3] = rng.integers(0, 2, size=n)
    t[4] = (1 - t[3]) * rng.integers(0, 2, size=n).astype(np.uint64)
    return t


def measure(lg_n, reps=5):
    config = p.StarkConfig.standard_fast_config()
    ctx = p.Context(0)
    sset = p.StarkSet(system(lg_n, config), ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(lg_n))
    chs = [int(v) for v in rng.integers(0, P, size=2 * NC, dtype=np.uint64)]
    alphas = [int(v) for v in rng.integers(0, P, size=NC, dtype=np.uint64)]
    traces = []
    sums = {"commit": [0.0] * reps, "ctl z": [0.0] * reps, "quotient": [0.0] * reps, "ctl quotient": [0.0] * reps}
    for table in range(3):
        trace = trace_of(rng, 1 << lg_n)
        traces.append(trace)
        for r in range(reps):
            ctx.timing(True)
            trace_b = p.PolynomialBatch.from_values(list(trace), config.rate_bits, False, config.cap_height, ctx=ctx)
            sums["commit"][r] += sum(v["ms"] for v in ctx.timing_report().values())
            ctx.timing(True)
            zs_b = sset.zs(table, trace, None, chs)
            sums["ctl z"][r] += ctx.timing_report()["compute CTL Z polys"]["ms"]
            ctx.timing(True)
            sset.quotient_polys(table, trace_b, zs_b, None, chs, alphas, []).free()
            rep = ctx.timing_report()
            sums["quotient"][r] += rep["compute quotient polys"]["ms"]
            sums["ctl quotient"][r] += rep["compute quotient polys (CTL checks)"]["ms"]
            zs_b.free()
            trace_b.free()
    sset.prove(traces)
    device, wall = [], []
    for _ in range(3):
        ctx.timing(True)
        t0 = time.perf_counter()
        sset.prove(traces)
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(sum(v["ms"] for v in ctx.timing_report().values()))
    ctx.timing(False)
    out = {k: 1e3 * statistics.median(v) for k, v in sums.items()}
    out.update(proof=1e3 * statistics.median(device), wall=statistics.median(wall))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, nargs="+", default=[16, 18, 20])
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["| rows per table | trace commitments (us) | CTL Z phase, 10 Zs (us) | quotient launch (us) | CTL pass of the quotient (us) | set proof, device scopes (us) | set proof, wall (ms) |",
             "|---|---|---|---|---|---|---|"]
    for lg_n in a.rows_log:
        m = measure(lg_n)
        lines.append("| 2^%d | %.1f | %.1f | %.1f | %.1f | %.1f | %.1f |" % (lg_n, m["commit"], m["ctl z"], m["quotient"], m["ctl quotient"], m["proof"], m["wall"]))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
