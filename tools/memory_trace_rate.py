#!/usr/bin/env python3
"""The device time of MemoryStark's trace generation against the host entry and against the commitment of the columns it fills (run
on the GPU).

    python tools/memory_trace_rate.py [--rows-log 16 20] [--out FILE]

Per height n = 2^16 and 2^20, for a log of n - n / 16 operations on n / 8 addresses whose gaps push some rows (the height stays n):
  - the device time of gl_memory_trace_new (upload of the log, the two sorts, the counts and their prefix sum; its one wait included)
    and of gl_memory_trace_fill (the rows, then the lookup's permuted columns), HIP events on the context's stream (gl_ctx_timing_*);
    the fill's own scope apart from the lookup's;
  - the device time of Stark.commit_trace's work, PolynomialBatch::from_values of the 26 columns under
    StarkConfig::standard_fast_config (rate_bits 1, cap_height 4), the sum of its outermost timing scopes (the NTT passes' own scopes nest inside them and are not
    added again);
  - the host time of gl_memory_trace_host for the same log on one thread, the median of three calls.
Every device figure is the median of 7 runs that follow one untimed run of the same call directly, all in one process.  Prints a
markdown table (profiles/README.md holds the one from the one run made).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 7
COMMIT_TOP_LEVEL = ("IFFT", "FFT + blinding", "merkle_leaf_hash", "merkle_levels")      # the outermost scopes of a commitment (batch.hip, merkle.hip)


def scopes_ms(ctx, call):
    """name -> median ms over REPS timed runs, after one untimed run"""
    call()
    runs = []
    for _ in range(REPS):
        ctx.timing(True)
        call()
        runs.append({k: v["ms"] for k, v in ctx.timing_report().items()})
    ctx.timing(False)
    return {k: statistics.median(r.get(k, 0.0) for r in runs) for k in runs[0]}


def make_log(p, n, seed):
    """n - n / 16 ops: per address a write and reads at increasing timestamps; a few far addresses and late reads push rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    num_ops = n - n // 16
    ops = np.zeros(num_ops, dtype=p.MEMORY_OP_DTYPE)
    ops["filter"] = 1
    ops["context"] = rng.integers(0, 4, size=num_ops)
    ops["segment"] = rng.integers(0, 8, size=num_ops)
    ops["virt"] = rng.integers(0, max(1, n // 256), size=num_ops)
    far = rng.random(num_ops) < 1.0 / 4096
    ops["virt"][far] += 3 * n                                          # a virt gap of about 3 n: three pushed rows
    ops["timestamp"] = rng.permutation(num_ops).astype(np.uint32) * 2
    ops["is_read"] = rng.integers(0, 2, size=num_ops)
    ops["value"] = rng.integers(0, 1 << 32, size=(num_ops, 8))          # any values: generation does not look at them
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--out")
    a = ap.parse_args()
    import plonky2_demo_amd as p
    ctx = p.Context(0)
    lines = ["| rows | ops | new: sort and count (ms) | fill: rows (ms) | fill: lookup columns (ms) | new + fill (ms) | commitment of the 26 columns (ms) | ratio | gl_memory_trace_host, one thread (ms) |",
             "|---|---|---|---|---|---|---|---|---|"]
    for lg_n in a.rows_log:
        n = 1 << lg_n
        ops = make_log(p, n, lg_n)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = p.memory_trace_host(ops)
            host.append(1e3 * (time.perf_counter() - t0))
        assert want.shape == (26, n), "the log's trace has %d rows, not 2^%d" % (want.shape[1], lg_n)
        d = ctx.alloc(26 * n * 8)
        try:
            def generate():
                t = p.MemoryTrace(ops, ctx=ctx)
                t.fill(d.ptr)
                t.close()
            ms = scopes_ms(ctx, generate)
            assert (d.download((26, n)) == want).all(), "the device and the host disagree"
            new_ms, rows_ms, lookup_ms = ms["memory trace: sort and count"], ms["memory trace: fill"] - ms["lookup columns"] if "lookup columns" in ms else ms["memory trace: fill"], ms.get("lookup columns", 0.0)
            scopes = scopes_ms(ctx, lambda: p.PolynomialBatch.from_device(d.ptr, 26, n, 1, 4, True, ctx=ctx).close())
            commit = sum(scopes[k] for k in COMMIT_TOP_LEVEL)           # scopes nest and are inclusive: the NTT passes stand inside the first two
            print("commitment scopes:", {k: round(v, 3) for k, v in scopes.items()}, flush=True)
        finally:
            d.free()
        total = new_ms + rows_ms + lookup_ms
        lines.append("| 2^%d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f | %.1f |" % (lg_n, ops.size, new_ms, rows_ms, lookup_ms, total, commit, total / commit,
                                                                                       statistics.median(host)))
        print(lines[-1], flush=True)
        print("scopes:", {k: round(v, 3) for k, v in ms.items()}, flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
