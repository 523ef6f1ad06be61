#!/usr/bin/env python3
"""Writes tests/golden/stark_fibonacci_n32.bin / .json (run on the GPU): the proof of the reference's test_fibonacci_stark shape -- 2^5
rows, x0 = 0, x1 = 1, StarkConfig::standard_fast_config -- which the CPU tests verify and tamper with (tests/test_stark_host.py) and the
GPU test holds current (tests/test_stark.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plonky2_demo_amd as p  # noqa: E402

NUM_ROWS, X0, X1 = 32, 0, 1


def main():
    desc, generate = p.fibonacci_stark(NUM_ROWS)
    config = p.StarkConfig.standard_fast_config()
    trace = generate(X0, X1)
    public_inputs = [X0, X1, int(trace[1, NUM_ROWS - 1])]
    stark = p.Stark(desc, config, NUM_ROWS.bit_length() - 1)
    proof = stark.prove(trace, public_inputs)
    ok, why, _ = stark.verify(proof)
    assert ok, why
    params = stark.params
    words = lambda off: [int.from_bytes(proof[off + 8 * i:off + 8 * i + 8], "little") for i in range(4)]      # noqa: E731
    cap_bytes = 32 << params.cap_height
    meta = {
        "air": "fibonacci", "num_rows": NUM_ROWS, "public_inputs": public_inputs, "num_challenges": config.num_challenges, "hasher": "poseidon",
        "params": {"degree_bits": params.degree_bits, "rate_bits": params.rate_bits, "cap_height": params.cap_height,
                   "proof_of_work_bits": params.proof_of_work_bits, "num_query_rounds": params.num_query_rounds,
                   "reduction_arity_bits": params.reduction_arity_bits},
        "num_bytes": len(proof),
        "trace_cap_first_words": words(0), "permutation_zs_cap_first_words": words(cap_bytes), "quotient_polys_cap_first_words": words(2 * cap_bytes),
    }
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "stark_fibonacci_n32.bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(golden, "stark_fibonacci_n32.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%d bytes, public inputs %s" % (len(proof), public_inputs))


if __name__ == "__main__":
    main()
