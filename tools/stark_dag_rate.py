#!/usr/bin/env python3
"""The device time of the quotient launch in both forms of a table's constraints -- k_stark_quotient on a term list against
k_stark_quotient_dag on the same AIR converted mechanically -- and, for an AIR only the DAG can hold, the quotient against the trace
commitment and proofs per second (run on the GPU).

    python tools/stark_dag_rate.py [--rows-log 16] [--sbox-rows-log 14] [--seconds 2.0] [--out FILE]

  - `nonic` (11 columns, degree 9, q = 8: a quotient coset of 8 n points, three pairs) and `wide` (130 columns, degree 2, q = 1, 131
    constraints) of tests/stark_airs.py at 2^rows-log rows, each as its term list and as tests/stark_dag_airs.py's conversion of it, on
    the SAME committed batches, the two forms alternating, medians (min .. max) of 9.  The traces are seeded random words: the quotient
    launch does not look whether the trace satisfies the AIR, and gl_stark_quotient_values does not check a degree.  The two outputs
    are compared word for word before anything is timed.
  - `sbox2` of tests/stark_dag_airs.py (12 columns, two rounds of x -> M (x + c)^3 per row, degree 9) at 2^sbox-rows-log rows on a
    satisfying trace, its proof verified once: the trace commitment (its IFFT, LDE and Merkle scopes), the quotient launch, proofs/s on
    one thread.
Device times are HIP events on the context's stream (gl_ctx_timing_*), every shape warmed up once.  Prints markdown tables
(profiles/README.md holds the ones from the one run made).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402

P = p.GOLDILOCKS_ORDER
QUOTIENT = "compute quotient polys"


def config_of(air, nc=2):
    c = p.StarkConfig.standard_fast_config()
    c.num_challenges, c.rate_bits = nc, air.rate_bits
    return c


def spread(xs):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def both_forms(name, lg_n, reps=9):
    import stark_airs
    import stark_dag_airs
    import stark_dag_model
    air, dag = stark_airs.AIRS[name], stark_dag_airs.CONVERTED[name]
    config, ctx = config_of(air), p.Context(0)
    terms = p.Stark(p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs), config, lg_n, ctx=ctx)
    desc = stark_dag_model.desc_of(p, dag)
    nodes = p.Stark(desc, config, lg_n, ctx=ctx)
    rng = np.random.Generator(np.random.PCG64(1))
    trace = rng.integers(0, P, size=(air.num_columns, 1 << lg_n), dtype=np.uint64)
    sets = rng.integers(0, P, size=air.q * config.num_challenges * 2, dtype=np.uint64) if air.pairs else None
    alphas, pis = [int(v) for v in rng.integers(0, P, size=2, dtype=np.uint64)], [int(v) for v in rng.integers(0, P, size=air.num_public_inputs, dtype=np.uint64)]
    trace_b = terms.commit_trace(list(trace))
    zs_b = terms.permutation_zs(trace, sets) if air.pairs else None
    args = (trace_b, zs_b, sets, alphas, pis)
    assert (terms.quotient_values(*args) == nodes.quotient_values(*args)).all(), "the two forms differ"       # and the warm-up of both
    times = {"term list": [], "DAG": []}
    for _ in range(reps):
        for form, stark in (("term list", terms), ("DAG", nodes)):
            ctx.timing(True)
            stark.quotient_values(*args)
            times[form].append(1e3 * ctx.timing_report()[QUOTIENT]["ms"])
    ctx.timing(False)
    max_live, _, instructions = desc.stats()
    num_terms = sum(len(t) for _, t in air.constraints)
    return ["| %s | term list | %d terms | -- | %s |" % (name, num_terms, spread(times["term list"])),
            "| %s | DAG | %d instructions | %d (%d B of LDS per workgroup) | %s |" % (name, instructions, max_live, 512 * max_live, spread(times["DAG"]))]


def sbox2(lg_n, seconds, reps=9):
    import stark_dag_airs
    import stark_dag_model
    dag = stark_dag_airs.sbox2
    config, ctx = config_of(dag), p.Context(0)
    desc = stark_dag_model.desc_of(p, dag)
    stark = p.Stark(desc, config, lg_n, ctx=ctx)
    trace, pis = dag.trace(1 << lg_n, seed=1)
    proof = stark.prove(trace, pis)
    assert stark.verify(proof) == (True, "", 0)
    commit, quot = [], []
    for _ in range(reps):
        ctx.timing(True)
        stark.commit_trace(list(trace)).free()
        commit.append(1e3 * sum(v["ms"] for v in ctx.timing_report().values()))
        ctx.timing(True)
        stark.prove(trace, pis)
        quot.append(1e3 * ctx.timing_report()[QUOTIENT]["ms"])
    ctx.timing(False)
    count, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        stark.prove(trace, pis)                                       # ends in the download of the proof: the stream is idle when it returns
        count += 1
    rate = count / (time.perf_counter() - t0)
    max_live, _, instructions = desc.stats()
    return "| sbox2 at 2^%d rows | %d | %d | %d | %s | %s | %.1f |" % (lg_n, len(proof), instructions, max_live, spread(commit), spread(quot), rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, default=16)
    ap.add_argument("--sbox-rows-log", type=int, default=14)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = ["| AIR at 2^%d rows | form | program | max live | quotient launch (us), median (min .. max) of 9 |" % a.rows_log, "|---|---|---|---|---|"]
    for name in ("nonic", "wide"):
        lines += both_forms(name, a.rows_log)
        print("\n".join(lines[-2:]), flush=True)
    lines += ["", "| AIR | proof bytes | instructions | max live | trace commitment (us) | quotient launch (us) | proofs/s, 1 thread |", "|---|---|---|---|---|---|---|",
              sbox2(a.sbox_rows_log, a.seconds)]
    text = "\n".join(lines) + "\n\nGPU_MAX_HW_QUEUES = %s\n" % os.environ.get("GPU_MAX_HW_QUEUES")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
