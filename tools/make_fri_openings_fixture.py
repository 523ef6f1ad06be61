#!/usr/bin/env python3
"""Regenerates tests/golden/fri_openings_n128.bin and .json (needs the GPU): a FriProof of the STARK-shaped instance of
tests/test_fri_openings.py (oracles of 7, 2 and 4 columns; all thirteen at zeta, the first two oracles at g zeta; n = 2^7, rate_bits 1,
cap_height 4, 16 bits of work) with 28 queries, and beside it what a verifier needs: params, instance, oracle caps, openings.
`out` defaults to tests/golden."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p
import test_fri_openings as t

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
ctx = p.default_context()
case = t.StarkCase((p, ctx), 7, "poseidon", num_queries=28)
assert case.library(p) == (True, "", 0), "fixture proof rejected"
fp = case.params
doc = {
    "params": {"degree_bits": fp.degree_bits, "rate_bits": fp.rate_bits, "cap_height": fp.cap_height, "proof_of_work_bits": fp.proof_of_work_bits,
               "num_query_rounds": fp.num_query_rounds, "reduction_arity_bits": fp.reduction_arity_bits, "hiding": bool(fp.hiding), "hasher": fp.hasher},
    "oracles": [[k, bool(b)] for k, b in case.instance.oracles],
    "batches": [[list(pt), [list(oc) for oc in polys]] for pt, polys in case.instance.batches],
    "caps": [[[int(w) for w in h] for h in cap] for cap in case.caps],
    "openings": [[int(a), int(b)] for a, b in case.openings],
}
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "fri_openings_n128.bin"), "wb") as f:
    f.write(case.proof)
with open(os.path.join(out, "fri_openings_n128.json"), "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("fixture written:", len(case.proof), "proof bytes")
