#!/usr/bin/env python3
"""Proofs/s of verification: gl_verify in a loop on one host core against gl_batch_verifier_verify at batch 1, 16, 64 and 256, with 1
and 16 host threads, for m = 64 proofs (host-stage heavy: 12288 public inputs = 1536 permutations of the public-input sponge) and
m = 8 proofs (192 public inputs).  Both sides are timed at the C ABI with the pointer arrays built beforehand, on the same proofs, in
one process; every timed window follows an untimed call of the same shape (run-in) and is repeated, median and spread reported.
    python tools/verify_rate.py [reps=7] [m ...]
Prints one table and one JSON line per row."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import plonky2_demo_amd as p
from plonky2_demo_amd._lib import lib, check

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
sizes = [int(a) for a in sys.argv[2:]] or [64, 8]
DISTINCT, BATCHES, THREADS = 16, (1, 16, 64, 256), (1, 16)
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def rate(count, call):
    """(median, min, max) proofs/s of `call`, which verifies `count` proofs and returns when they are judged"""
    call()                                               # run-in, directly in front of the timed repetitions
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(count / (time.perf_counter() - t0))
    return statistics.median(out), min(out), max(out)


rows = []
for m in sizes:
    hc = p.MatmulCircuit(m)
    rng = np.random.default_rng(m)
    ops = [(rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64), rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)) for _ in range(DISTINCT)]
    pool = p.ProverPool(hc, lanes=4)
    distinct = [pr.to_bytes() for pr in pool.prove_matmul(ops)]
    cap, dig = np.ascontiguousarray(pool.constants_sigmas_cap), np.ascontiguousarray(pool.circuit_digest)
    proofs = [distinct[i % DISTINCT] for i in range(max(BATCHES))]
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in proofs]
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * len(bufs))(*[b.size for b in bufs])
    desc = hc.desc

    def host_loop(count=64):
        for i in range(count):
            check(lib.gl_verify(ctypes.byref(desc), vp(cap), vp(dig), ptrs[i], lens[i]))
    med, lo, hi = rate(64, host_loop)
    host = med
    rows.append({"m": m, "path": "gl_verify loop", "host_threads": 1, "batch": 1, "proofs_per_s": med, "min": lo, "max": hi, "gain": 1.0})
    ctx = p.default_context()
    for threads in THREADS:
        for batch in BATCHES:
            bv = p.BatchVerifier(desc, cap, dig, ctx=ctx, max_batch=batch, host_threads=threads)
            verdicts, checks = np.full(batch, -1, dtype=np.int32), np.zeros(batch, dtype=np.uint32)

            def batch_call():
                check(lib.gl_batch_verifier_verify(bv.handle, ptrs, lens, batch, vp(verdicts), vp(checks)))
            med, lo, hi = rate(batch, batch_call)
            assert not verdicts.any() and not checks.any(), "a valid proof was rejected"
            rows.append({"m": m, "path": "gl_batch_verifier_verify", "host_threads": threads, "batch": batch, "proofs_per_s": med, "min": lo, "max": hi,
                         "gain": med / host})
            bv.close()

print("%-4s %-26s %7s %6s %12s %21s %6s" % ("m", "path", "threads", "batch", "proofs/s", "min .. max", "gain"))
for r in rows:
    print("%-4d %-26s %7d %6d %12.1f %9.1f .. %-9.1f %5.2fx" % (r["m"], r["path"], r["host_threads"], r["batch"], r["proofs_per_s"], r["min"], r["max"], r["gain"]))
for r in rows:
    print(json.dumps(r))
