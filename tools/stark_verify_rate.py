#!/usr/bin/env python3
"""Proofs/s of STARK verification: gl_stark_verify in a loop on 1 and on 16 host threads against gl_stark_batch_verifier_verify at
batch 1, 16, 64 and 256 with 1 and 16 host threads, for the `fibonacci` AIR (4 columns) and the `wide` AIR (130 columns: 17
permutations per trace leaf) of tests/stark_airs.py at 2^12 rows under standard_fast_config (84 queries, two reductions).  Both sides
are timed at the C ABI with the pointer arrays built beforehand, on the same 16 distinct proofs, cycled, in one process; the batch
call returns after the device has answered (it waits for its stream).  Every timed window follows an untimed call of the same shape
(run-in) and is repeated, median and spread reported.
    python tools/stark_verify_rate.py [reps=7] [lg_n=12] [air ...]
Prints one table and one JSON line per row."""
import ctypes, json, os, statistics, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import plonky2_demo_amd as p
import stark_airs
from plonky2_demo_amd._lib import lib, check

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
lg_n = int(sys.argv[2]) if len(sys.argv) > 2 else 12
names = sys.argv[3:] or ["fibonacci", "wide"]
DISTINCT, BATCHES, THREADS, LOOP = 16, (1, 16, 64, 256), (1, 16), 64
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
ctx = p.default_context()
for name in names:
    air = stark_airs.AIRS[name]
    config = p.StarkConfig.standard_fast_config()
    config.rate_bits = air.rate_bits
    desc = p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs)
    stark = p.Stark(desc, config, lg_n, ctx=ctx)
    n = 1 << lg_n
    traces = [air.trace(n, 0, k, 2 * k + 1) if name == "fibonacci" else air.trace(n, seed=k) for k in range(DISTINCT)]
    distinct = [stark.prove(trace, pis) for trace, pis in traces]
    assert len(set(distinct)) == DISTINCT
    proofs = [distinct[i % DISTINCT] for i in range(max(BATCHES))]
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in proofs]
    ptrs = (ctypes.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * len(bufs))(*[b.size for b in bufs])
    st, params = desc.struct(config.num_challenges), stark.params

    def host_range(first, last):
        for i in range(first, last):
            check(lib.gl_stark_verify(ctypes.byref(st), ctypes.byref(params), ptrs[i], lens[i], None))

    def host_threads(threads):
        """the LOOP proofs split over `threads` threads (ctypes drops the interpreter lock inside a call)"""
        def call():
            if threads == 1:
                return host_range(0, LOOP)
            ts = [threading.Thread(target=host_range, args=(LOOP * k // threads, LOOP * (k + 1) // threads)) for k in range(threads)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
        return call
    host = {}
    for threads in THREADS:
        med, lo, hi = rate(LOOP, host_threads(threads))
        host[threads] = med
        rows.append({"air": name, "lg_n": lg_n, "proof_bytes": len(distinct[0]), "path": "gl_stark_verify loop", "host_threads": threads, "batch": 1,
                     "proofs_per_s": med, "min": lo, "max": hi, "gain": 1.0})
    for threads in THREADS:
        for batch in BATCHES:
            bv = p.StarkBatchVerifier(desc, config, lg_n, ctx=ctx, max_batch=batch, host_threads=threads)
            verdicts, checks = np.full(batch, -1, dtype=np.int32), np.zeros(batch, dtype=np.uint32)

            calls = max(1, LOOP // batch)                  # a window judges at least as many proofs as the loop's

            def batch_call():
                for _ in range(calls):
                    check(lib.gl_stark_batch_verifier_verify(bv.handle, ptrs, lens, batch, vp(verdicts), vp(checks)))
            med, lo, hi = rate(batch * calls, batch_call)
            assert not verdicts.any() and not checks.any(), "a valid proof was rejected"
            rows.append({"air": name, "lg_n": lg_n, "proof_bytes": len(distinct[0]), "path": "gl_stark_batch_verifier_verify", "host_threads": threads,
                         "batch": batch, "proofs_per_s": med, "min": lo, "max": hi, "gain": med / host[threads]})      # against the loop on as many threads
            bv.close()
    stark.close()

print("%-10s %-32s %7s %6s %12s %21s %6s" % ("air", "path", "threads", "batch", "proofs/s", "min .. max", "gain"))
for r in rows:
    print("%-10s %-32s %7d %6d %12.1f %9.1f .. %-9.1f %5.2fx" % (r["air"], r["path"], r["host_threads"], r["batch"], r["proofs_per_s"], r["min"], r["max"], r["gain"]))
for r in rows:
    print(json.dumps(r))
