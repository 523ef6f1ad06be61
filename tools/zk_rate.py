#!/usr/bin/env python3
"""Proofs/s of the matmul prover pool (gl_prover_pool_prove_matmul: device witness generation, then proving) for the plain and the
zero-knowledge build of one m; a zk item also blinds its witness (gl_witness_blind) and salts three commitments.
    python tools/zk_rate.py m {plain|zk} [count=320] [lanes=16]
Run the legs of one comparison in the same GPU session, each in its own process under a time limit, e.g.
    for m in 64 128; do for k in plain zk; do timeout -k 10 300 python tools/zk_rate.py $m $k || break 2; done; done"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
import numpy as np
import plonky2_demo_amd as p

m = int(sys.argv[1]) if len(sys.argv) > 1 else 64
zk = (sys.argv[2] if len(sys.argv) > 2 else "plain") == "zk"
count = int(sys.argv[3]) if len(sys.argv) > 3 else 320
lanes = int(sys.argv[4]) if len(sys.argv) > 4 else 16
hc = p.MatmulCircuit(m, zero_knowledge=zk)
rng = np.random.default_rng(1)
ops = [(rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64), rng.integers(0, 2**32 - 1, m * m, dtype=np.uint64)) for _ in range(4)]
pool = p.ProverPool(hc, lanes=lanes)
warm = pool.prove_matmul([ops[i % 4] for i in range(2 * lanes)])       # warm-up batch: code objects, tables, pools
t0 = time.perf_counter()
proofs = pool.prove_matmul([ops[i % 4] for i in range(count)])
dt = time.perf_counter() - t0
cap, dig = pool.constants_sigmas_cap, pool.circuit_digest
ok = all(hc.verify(proofs[i].to_bytes(), cap, dig)[0] for i in range(0, count, max(1, count // 8)))
print("m = %d %s (n = 2^%d), %d lanes: %d proofs in %.3f s = %.1f proofs/s (sampled proofs verify: %s)"
      % (m, "zk" if zk else "plain", hc.desc.degree_bits, lanes, count, dt, count / dt, ok))
