#!/usr/bin/env python3
"""Regenerates tests/golden/ext_gates_n8_proof.bin and ext_gates_n8_verifier_only.bin (needs the GPU): one proof of the n = 8 circuit with
one row of each of the four extension-field arithmetic gates (tests/test_ext_gates.py::_fixture_circuit) and the circuit's
VerifierOnlyCircuitData bytes (constants_sigmas_cap + circuit digest).  `out` defaults to tests/golden."""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import plonky2_demo_amd as p
from plonky2_demo_amd import api
import test_ext_gates as t

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
c = t._fixture_circuit()
cd = t._build(p, c, p.default_context())
proof = cd.prove(c.wires(), np.zeros(0, dtype=np.uint64)).to_bytes()
assert cd.verify(proof) == (True, ""), "fixture proof rejected"
vo = api.verifier_only_to_bytes(cd.constants_sigmas_cap, cd.circuit_digest)
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, "ext_gates_n8_proof.bin"), "wb") as f:
    f.write(proof)
with open(os.path.join(out, "ext_gates_n8_verifier_only.bin"), "wb") as f:
    f.write(vo)
print("fixture written:", len(proof), "proof bytes,", len(vo), "verifier-only bytes")
