#!/usr/bin/env python3
"""Writes the committed zero-knowledge proof tests/golden/zk_matmul2_n256.bin / .json (run on the GPU): the 2 x 2 matmul circuit as a
zero-knowledge build with one query round (n = 256, one FRI reduction, Poseidon), blinded and proved under one seed.  The CPU test
tests/test_zk_model_host.py derives the same bytes from plain integers (tests/zk_model.py), has gl_verify accept them and both verifiers
reject the same tampered copies; tests/test_zk_model.py holds the fixture current on the GPU.

--out DIR writes there instead of tests/golden."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402
import zk_circuits as zc  # noqa: E402

STEM = "zk_matmul2_n256"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    (_, m, operand_seed, filler_seed), hasher, queries, pow_bits, seed, n, rounds = zc.CASES[zc.FIXTURE_CASE]
    a, b = zc.matmul_operands(m, operand_seed)
    zd, cs, wires, pis, seed = zc.build_case(p, None, zc.FIXTURE_CASE)
    ctx = p.default_context()
    cd = p.GenericCircuitData(zd, cs, ctx=ctx)
    buf = ctx.alloc(wires.nbytes)
    buf.upload(wires)
    cd.blind_witness(buf.ptr, seed=seed)
    proof = cd.prove_device(buf.ptr, pis, seed=seed).to_bytes()
    buf.free()
    ok, why = cd.verify(proof)
    assert ok, why
    meta = {"circuit": "matmul", "m": m, "a": [int(v) for v in a], "b": [int(v) for v in b], "filler_seed": filler_seed, "salt_seed": seed.hex(),
            "num_query_rounds": queries, "proof_of_work_bits": pow_bits, "hasher": hasher, "degree_bits": zd.degree_bits,
            "num_gate_rows": zd.num_gate_rows, "num_fri_rounds": zd.num_fri_rounds, "num_bytes": len(proof)}
    with open(os.path.join(args.out, STEM + ".bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(args.out, STEM + ".json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%s: %d bytes, n = %d, %d query round(s)" % (STEM, len(proof), 1 << zd.degree_bits, queries))


if __name__ == "__main__":
    main()
