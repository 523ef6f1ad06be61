#!/usr/bin/env python3
"""Writes the committed proof of a STARK table in DAG form, tests/golden/stark_dag_sbox2_n32.bin / .json (run on the GPU): sbox2 of
tests/stark_dag_airs.py -- an AIR the term list cannot hold -- at 2^5 rows under two challenges, degree 9 at rate_bits 3.  The CPU tests
verify and tamper with it (tests/test_stark_dag_host.py) and a GPU test holds it current (tests/test_stark_dag.py).

--out DIR writes there instead of tests/golden."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402

STEM, NUM_ROWS, NUM_CHALLENGES, SEED = "stark_dag_sbox2_n32", 32, 2, 9


def main():
    import stark_dag_airs
    import stark_dag_model
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    air = stark_dag_airs.sbox2
    config = p.StarkConfig.standard_fast_config()
    config.num_challenges, config.rate_bits = NUM_CHALLENGES, air.rate_bits
    trace, public_inputs = air.trace(NUM_ROWS, seed=SEED)
    stark = p.Stark(stark_dag_model.desc_of(p, air), config, NUM_ROWS.bit_length() - 1)
    proof = stark.prove(trace, public_inputs)
    ok, why, _ = stark.verify(proof)
    assert ok, why
    params = stark.params
    words = lambda off: [int.from_bytes(proof[off + 8 * i:off + 8 * i + 8], "little") for i in range(4)]      # noqa: E731
    cap_bytes = 32 << params.cap_height
    meta = {
        "air": air.name, "num_rows": NUM_ROWS, "public_inputs": public_inputs, "num_challenges": NUM_CHALLENGES, "hasher": "poseidon", "trace_seed": SEED,
        "params": {"degree_bits": params.degree_bits, "rate_bits": params.rate_bits, "cap_height": params.cap_height,
                   "proof_of_work_bits": params.proof_of_work_bits, "num_query_rounds": params.num_query_rounds,
                   "reduction_arity_bits": params.reduction_arity_bits},
        "num_bytes": len(proof), "trace_cap_first_words": words(0), "quotient_polys_cap_first_words": words(cap_bytes),
    }
    with open(os.path.join(args.out, STEM + ".bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(args.out, STEM + ".json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%s: %d bytes" % (STEM, len(proof)))


if __name__ == "__main__":
    main()
