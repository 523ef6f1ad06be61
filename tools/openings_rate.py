#!/usr/bin/env python3
"""Device time of the stage "reduce batches + divide" of prove_openings, one pass over the distinct columns (k_fri_combine_points,
k_div_points_*: gl_fri_combine_instance) against one pass per batch (k_fri_combine, k_div_linear_*), on one GPU in one process, the two
taken alternately.  Timed with the context's device events (gl_ctx_timing_*: one event pair around the stage's launches); each window
of `inner` alternating pairs follows an untimed run-in of the same pairs (~50 ms of the same work, profiles/README.md), and is repeated
`reps` times: median, min and max of the per-call means.
  (a) the m = 64 Plonk instance (everything at zeta, the two Z polynomials at g zeta): gl_fri_combine_instance against the same instance
      through gl_fri_combine_instance_per_batch (the sequence gl_fri_combine ran before it became a caller of the one-pass kernels);
      gl_fri_combine itself is held equal to both first
  (b) a STARK-shaped instance a user would run (n = 2^20, rate_bits 1, 128 + 2 + 4 columns, the first two oracles opened twice):
      gl_fri_combine_instance against the same instance through gl_fri_combine_instance_per_batch
    python tools/openings_rate.py [reps=9] [inner=20]
Prints one table and one JSON line per row."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import plonky2_demo_amd as p

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 20
P = p.GOLDILOCKS_ORDER
OLD_PER_BATCH, NEW = "reduce batch + divide by linear, batch after batch", "reduce batches + divide by linear"
ctx = p.default_context()


def measure(old, new, old_scope):
    """old(), new(): one combine each (the gl_fri is dropped at once) -> {path: (median, min, max) us per call}"""
    def pairs(k):
        for _ in range(k):
            old().close()
            new().close()
    ctx.timing(False)
    pairs(max(inner, 8))                                  # run-in: the same work, untimed, directly in front
    per_call = {old_scope: [], NEW: []}
    for _ in range(reps):
        ctx.timing(True)
        pairs(inner)
        rep = ctx.timing_report()
        for scope in per_call:
            assert rep[scope]["count"] == inner, rep
            per_call[scope].append(1e3 * rep[scope]["ms"] / inner)
    ctx.timing(False)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in per_call.items()}


rows = []
# (a) the m = 64 Plonk instance
hc = p.MatmulCircuit(64)
cd = hc.build(ctx)
d = cd.desc
n = 1 << d.degree_bits
rng = np.random.default_rng(64)
wires, pis = hc.witness(rng.integers(0, 2**32 - 1, 64 * 64, dtype=np.uint64), rng.integers(0, 2**32 - 1, 64 * 64, dtype=np.uint64), filler_seed=1)
d_w = ctx.alloc(wires.nbytes).upload(wires)
wires_b = p.PolynomialBatch.from_device(d_w.ptr, 135, n, d.rate_bits, d.cap_height, True, ctx=ctx)
zs_b = cd.partial_products(d_w.ptr, [3, 4], [5, 6], ctx=ctx)
q_b = cd.quotient_polys(wires_b, zs_b, [1, 2, 3, 4], [3, 4], [5, 6], [7, 8], ctx=ctx)
batches = [cd.constants_sigmas_batch, wires_b, zs_b, q_b]
zeta, alpha = [123456789, 987654321], [1111111, 2222222]
g = pow(7, (P - 1) >> d.degree_bits, P)
ncs = d.num_constants + 80
names = [[(o, c) for c in range(w)] for o, w in enumerate((ncs, 135, 20, 16))]
inst = p.FriInstance([(ncs, False), (135, False), (20, False), (16, False)],
                     [(zeta, names[0] + names[1] + names[2] + names[3]), ([zeta[0] * g % P, zeta[1] * g % P], names[2][:2])])
params = p.FriParams.of_circuit(d)
a_plonk, a_old, a_new = [cd.fri(batches, zeta, alpha, ctx=ctx)] + [p.FriProver.from_instance(inst, batches, alpha, params, ctx=ctx, per_batch=pb) for pb in (True, False)]
for _ in range(d.num_fri_rounds):
    cap = a_plonk.commit_round()
    assert (a_old.commit_round() == cap).all() and (a_new.commit_round() == cap).all()
    a_plonk.fold([9, 9]); a_old.fold([9, 9]); a_new.fold([9, 9])
assert (a_old.final_poly() == a_new.final_poly()).all() and (a_plonk.final_poly() == a_new.final_poly()).all(), "the paths differ"
a_plonk.close(); a_old.close(); a_new.close()
res = measure(lambda: p.FriProver.from_instance(inst, batches, alpha, params, ctx=ctx, per_batch=True),
              lambda: p.FriProver.from_instance(inst, batches, alpha, params, ctx=ctx), OLD_PER_BATCH)
rows.append({"shape": "(a) Plonk m = 64, n = 2^%d, %d + 2 openings" % (d.degree_bits, ncs + 171), "old": "per-batch sequence", "old_us": res[OLD_PER_BATCH], "new_us": res[NEW]})

# (b) a STARK-shaped instance
lg = 20
widths = [128, 2, 4]
cols = [rng.integers(0, P, (w, 1 << lg), dtype=np.uint64) for w in widths]
sb = [p.PolynomialBatch.from_coeffs(c, 1, False, 4, ctx=ctx) for c in cols]
del cols
g = pow(7, (P - 1) >> lg, P)
everything = [(o, c) for o, w in enumerate(widths) for c in range(w)]
sinst = p.FriInstance([(w, False) for w in widths], [(zeta, everything), ([zeta[0] * g % P, zeta[1] * g % P], [oc for oc in everything if oc[0] < 2])])
sparams = p.FriParams(lg, 1, 4, 16, 84, [4, 4, 4, 4])
b_old, b_new = (p.FriProver.from_instance(sinst, sb, alpha, sparams, ctx=ctx, per_batch=pb) for pb in (True, False))
for _ in range(4):
    assert (b_old.commit_round() == b_new.commit_round()).all()
    b_old.fold([9, 9]); b_new.fold([9, 9])
assert (b_old.final_poly() == b_new.final_poly()).all(), "the two paths differ"
b_old.close(); b_new.close()
res = measure(lambda: p.FriProver.from_instance(sinst, sb, alpha, sparams, ctx=ctx, per_batch=True),
              lambda: p.FriProver.from_instance(sinst, sb, alpha, sparams, ctx=ctx), OLD_PER_BATCH)
rows.append({"shape": "(b) STARK-shaped, n = 2^20, 134 + 130 openings", "old": "per-batch sequence", "old_us": res[OLD_PER_BATCH], "new_us": res[NEW]})

print("reps %d, %d alternating pairs per window; us per call: median (min .. max)" % (reps, inner))
print("%-50s %-20s %30s %30s %7s" % ("shape", "old path", "old", "one pass", "old/new"))
for r in rows:
    fmt = lambda t: "%9.1f (%8.1f .. %-8.1f)" % t
    print("%-50s %-20s %30s %30s %6.2fx" % (r["shape"], r["old"], fmt(r["old_us"]), fmt(r["new_us"]), r["old_us"][0] / r["new_us"][0]))
for r in rows:
    print(json.dumps(r))
