#!/usr/bin/env python3
"""STARK proofs per second and the device time of the two STARK kernels against the trace commitment (run on the GPU).

    python tools/stark_rate.py [--rows-log 16] [--seconds 2.0] [--out FILE]

Two AIRs at 2^16 rows under StarkConfig::standard_fast_config: `fibonacci` (4 columns, degree 2, q = 1, two Z polynomials) and a
synthetic 64-column degree-3 AIR (62 columns x_c' = x_c^2 x_(c+1) + c, one permutation pair on the other two; q = 2, one Z polynomial).
  - proofs/s with 1 and with 16 threads, one context (one stream) and one gl_stark each, every proof verified once beforehand;
  - per proof the device time (HIP events on the context's stream, gl_ctx_timing_*) of the permutation-Z launches and of the quotient
    launch, against the trace commitment of the same proof (its IFFT, LDE and Merkle scopes, timed on their own).
Prints a markdown table (profiles/README.md holds the one from the one run made).
"""
import argparse
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")       # one hardware queue per stream, unless the environment sets a value of its own
# (read when the HIP runtime initialises; the value in force is printed with the table)
import plonky2_demo_amd as p  # noqa: E402

P = p.GOLDILOCKS_ORDER
L, N, PUB = p.GL_STARK_LOCAL, p.GL_STARK_NEXT, p.GL_STARK_PUBLIC
STATE = 62


def synthetic(n, seed=1):
    """(description, trace [64][n], public inputs) of the 64-column degree-3 AIR"""
    constraints = [(p.GL_STARK_FIRST_ROW, [(1, [(L, 0)]), (P - 1, [(PUB, 0)])])]
    constraints += [(p.GL_STARK_TRANSITION, [(1, [(N, c)]), (P - 1, [(L, c), (L, c), (L, (c + 1) % STATE)]), ((P - c) % P, [])]) for c in range(STATE)]
    desc = p.StarkDesc(64, 1, 3, constraints, [[(62, 63)]])
    rng = np.random.Generator(np.random.PCG64(seed))
    row = [int(v) for v in rng.integers(0, P, size=STATE, dtype=np.uint64)]
    trace = np.empty((64, n), dtype=np.uint64)
    for i in range(n):
        trace[:STATE, i] = row
        row = [(row[c] * row[c] % P * row[(c + 1) % STATE] + c) % P for c in range(STATE)]
    trace[62] = rng.integers(0, P, size=n, dtype=np.uint64)
    trace[63] = trace[62][rng.permutation(n)]
    return desc, trace, [int(trace[0, 0])]


def fibonacci(n):
    desc, generate = p.fibonacci_stark(n)
    trace = generate(0, 1)
    return desc, trace, [0, 1, int(trace[1, n - 1])]


def rate(desc, config, lg_n, trace, pis, threads, seconds):
    """proofs/s over `threads` threads, each with its own context and gl_stark, after one untimed proof each"""
    counts, errors, start = [0] * threads, [], threading.Barrier(threads + 1)

    def work(i):
        try:
            ctx = p.Context(0)
            stark = p.Stark(desc, config, lg_n, ctx=ctx)
            stark.prove(trace, pis)
            start.wait()
            end = time.perf_counter() + seconds
            while time.perf_counter() < end:
                stark.prove(trace, pis)
                counts[i] += 1
        except Exception as e:                          # noqa: BLE001
            errors.append(e)
            start.abort()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
    for t in ts:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    if errors:
        raise errors[0]
    return sum(counts) / (time.perf_counter() - t0)


def device_times(desc, config, lg_n, trace, pis, reps=9):
    """median microseconds per proof: (trace commitment, permutation-Z launches, quotient launch)"""
    ctx = p.Context(0)
    stark = p.Stark(desc, config, lg_n, ctx=ctx)
    proof = stark.prove(trace, pis)
    assert stark.verify(proof) == (True, "", 0)
    commit, zs, quot = [], [], []
    for _ in range(reps):
        ctx.timing(True)
        stark.commit_trace(list(trace)).free()
        commit.append(1e3 * sum(v["ms"] for v in ctx.timing_report().values()))
        ctx.timing(True)
        stark.prove(trace, pis)
        rep = ctx.timing_report()
        zs.append(1e3 * rep["compute permutation Z polys"]["ms"])
        quot.append(1e3 * rep["compute quotient polys"]["ms"])
    ctx.timing(False)
    return statistics.median(commit), statistics.median(zs), statistics.median(quot), len(proof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, config = 1 << a.rows_log, p.StarkConfig.standard_fast_config()
    lines = ["| AIR at 2^%d rows | proof bytes | proofs/s, 1 thread | proofs/s, 16 threads | trace commitment (us) | permutation Z, 4 launches (us) | quotient, 1 launch (us) |" % a.rows_log,
             "|---|---|---|---|---|---|---|"]
    for name, (desc, trace, pis) in (("fibonacci", fibonacci(n)), ("synthetic 64 columns, degree 3", synthetic(n))):
        commit, zs, quot, size = device_times(desc, config, a.rows_log, trace, pis)
        r1 = rate(desc, config, a.rows_log, trace, pis, 1, a.seconds)
        r16 = rate(desc, config, a.rows_log, trace, pis, 16, a.seconds)
        lines.append("| %s | %d | %.1f | %.1f | %.1f | %.1f | %.1f |" % (name, size, r1, r16, commit, zs, quot))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n\nGPU_MAX_HW_QUEUES = %s\n" % os.environ.get("GPU_MAX_HW_QUEUES")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
