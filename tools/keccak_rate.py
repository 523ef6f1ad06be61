#!/usr/bin/env python3
"""Proofs/s of the matmul prover pool (gl_prover_pool_prove_matmul: device witness generation, then proving) under PoseidonGoldilocksConfig
and under KeccakGoldilocksConfig for one m, and with `latency` the wall time of single proofs on one context.
    python tools/keccak_rate.py m {poseidon|keccak} [count=320] [lanes=16] [latency]
Run the legs of one comparison in the same GPU session, alternating, each in its own process under a time limit, e.g.
    for r in 1 2 3; do for h in poseidon keccak; do timeout -k 10 300 python tools/keccak_rate.py 64 $h || break 2; done; done"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
import numpy as np
import plonky2_demo_amd as p

m = int(sys.argv[1]) if len(sys.argv) > 1 else 64
hasher = sys.argv[2] if len(sys.argv) > 2 else "poseidon"
count = int(sys.argv[3]) if len(sys.argv) > 3 else 320
lanes = int(sys.argv[4]) if len(sys.argv) > 4 else 16
hc = p.MatmulCircuit(m, hasher=hasher)
rng = np.random.default_rng(1)
ops = [(rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64), rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)) for _ in range(4)]
if len(sys.argv) > 5 and sys.argv[5] == "latency":
    ctx = p.default_context()
    cd = hc.build(ctx)
    cd.warm_up()
    gen = hc.witness_generator(ctx)
    buf = ctx.alloc(135 * hc.n * 8)
    pis = gen.run(ops[0][0], ops[0][1], buf.ptr, filler_seed=5)
    times = []
    for _ in range(count):
        t0 = time.perf_counter()
        proof = cd.prove_device(buf.ptr, pis, gen.public_inputs_hash)
        times.append(time.perf_counter() - t0)
    ok = cd.verify(proof)[0]
    times.sort()
    print("m = %d %s (n = 2^%d), one proof at a time: median %.3f ms, fastest %.3f ms of %d (verifies: %s)"
          % (m, hasher, hc.desc.degree_bits, 1e3 * times[len(times) // 2], 1e3 * times[0], count, ok))
    sys.exit(0 if ok else 1)
pool = p.ProverPool(hc, lanes=lanes)
warm = pool.prove_matmul([ops[i % 4] for i in range(2 * lanes)])       # warm-up batch: code objects, tables, pools
t0 = time.perf_counter()
proofs = pool.prove_matmul([ops[i % 4] for i in range(count)])
dt = time.perf_counter() - t0
cap, dig = pool.constants_sigmas_cap, pool.circuit_digest
ok = all(hc.verify(proofs[i].to_bytes(), cap, dig)[0] for i in range(0, count, max(1, count // 8)))
print("m = %d %s (n = 2^%d), %d lanes: %d proofs in %.3f s = %.1f proofs/s (sampled proofs verify: %s)"
      % (m, hasher, hc.desc.degree_bits, lanes, count, dt, count / dt, ok))
sys.exit(0 if ok else 1)
