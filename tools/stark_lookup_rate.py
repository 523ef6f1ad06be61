#!/usr/bin/env python3
"""The device time of gl_stark_lookup_columns against the commitment of the columns it fills and against the host (run on the GPU).

    python tools/stark_lookup_rate.py [--rows-log 16 20] [--counts 1 16 100] [--sort loop|segmented] [--out FILE]

Per call of 1, 16 and 100 lookups at n = 2^16 and 2^20, every lookup with an input column of its own against ONE shared counter column
0 .. n - 1 (ArithmeticStark::generate_range_checks' shape; the inputs are uniform in [0, n)):
  - the device time of the call (HIP events on the context's stream, gl_ctx_timing_*: the scope "lookup columns");
  - the device time of PolynomialBatch::from_values of the 2 x count columns the call fills, under StarkConfig::standard_fast_config
    (rate_bits 1, cap_height 4), the yardstick of tools/stark_rate.py and tools/stark_ctl_rate.py;
  - the host time of gl_permuted_cols_host for the same lookups on one thread: the median of three calls for one lookup, times count.
Every timed figure is the median of 7 runs that follow one untimed run of the same call directly.  --sort sets the tuning knob
GL_LOOKUP_SEGMENTED_SORT for the column sorts (DESIGN.md section 19 has both).  Prints a markdown table (profiles/README.md holds the
one from the one run made).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 7


def device_ms(ctx, call):
    call()                                              # the run-in, directly before the timed runs
    out = []
    for _ in range(REPS):
        ctx.timing(True)
        call()
        out.append(sum(v["ms"] for v in ctx.timing_report().values()))
    ctx.timing(False)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 16, 100])
    ap.add_argument("--sort", choices=["loop", "segmented"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.sort:
        os.environ["GL_LOOKUP_SEGMENTED_SORT"] = "1" if a.sort == "segmented" else "0"      # read at the first call
    import plonky2_demo_amd as p
    ctx = p.Context(0)
    lines = ["| rows | lookups | gl_stark_lookup_columns (ms) | commitment of the 2 x lookups columns (ms) | ratio | gl_permuted_cols_host, one thread (ms) |",
             "|---|---|---|---|---|---|"]
    for lg_n in a.rows_log:
        n = 1 << lg_n
        rng = np.random.Generator(np.random.PCG64(lg_n))
        table = np.arange(n, dtype=np.uint64)
        first = rng.integers(0, n, size=n, dtype=np.uint64)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = p.permuted_cols_host(first, table)
            host.append(1e3 * (time.perf_counter() - t0))
        host_ms = statistics.median(host)
        for count in a.counts:
            d = ctx.alloc((1 + 3 * count) * n * 8)
            try:
                d.upload(table)
                p._lib.check(p._lib.lib.gl_copy_h2d(ctx.handle, d.ptr + n * 8, first.ctypes.data, first.nbytes))
                for k in range(1, count):
                    col = rng.integers(0, n, size=n, dtype=np.uint64)
                    p._lib.check(p._lib.lib.gl_copy_h2d(ctx.handle, d.ptr + (1 + k) * n * 8, col.ctypes.data, col.nbytes))
                lookups = [(1 + k, 0, 1 + count + 2 * k, 2 + count + 2 * k) for k in range(count)]
                fill = device_ms(ctx, lambda: ctx.lookup_columns(d.ptr, 1 + 3 * count, n, lookups))
                got = np.empty((2, n), dtype=np.uint64)
                p._lib.check(p._lib.lib.gl_copy_d2h(ctx.handle, got.ctypes.data, d.ptr + (1 + count) * n * 8, got.nbytes))
                assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), "the device and the host disagree"
                commit = device_ms(ctx, lambda: p.PolynomialBatch.from_device(d.ptr + (1 + count) * n * 8, 2 * count, n, 1, 4, True, ctx=ctx).close())
            finally:
                d.free()
            lines.append("| 2^%d | %d | %.3f | %.3f | %.2f | %.1f |" % (lg_n, count, fill, commit, fill / commit, host_ms * count))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n\ncolumn sorts: %s\n" % (a.sort or "default")
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
