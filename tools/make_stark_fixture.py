#!/usr/bin/env python3
"""Writes a committed STARK proof, tests/golden/<fixture>.bin / .json (run on the GPU), which the CPU tests verify and tamper with
(tests/test_stark_host.py) and a GPU test holds current (tests/test_stark.py):

  make_stark_fixture.py [fibonacci]   stark_fibonacci_n32: the reference's test_fibonacci_stark shape -- 2^5 rows, x0 = 0, x1 = 1,
                                      StarkConfig::standard_fast_config (two challenges, q = 1)
  make_stark_fixture.py nonic         stark_nonic_n32_nc3: tests/stark_airs.py's nonic -- 2^5 rows, three challenges, degree 9 at
                                      rate_bits 3 (q = 8 chunks per challenge, two Z polynomials, the second of one instance)

--out DIR writes there instead of tests/golden."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402

NUM_ROWS, X0, X1 = 32, 0, 1
NONIC_CHALLENGES, NONIC_SEED = 3, 9


def fibonacci():
    desc, generate = p.fibonacci_stark(NUM_ROWS)
    trace = generate(X0, X1)
    return "stark_fibonacci_n32", "fibonacci", desc, p.StarkConfig.standard_fast_config(), trace, [X0, X1, int(trace[1, NUM_ROWS - 1])], {}


def nonic():
    import stark_airs
    air = stark_airs.nonic
    config = p.StarkConfig.standard_fast_config()
    config.num_challenges, config.rate_bits = NONIC_CHALLENGES, air.rate_bits
    trace, public_inputs = air.trace(NUM_ROWS, seed=NONIC_SEED)
    desc = p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs)
    return "stark_nonic_n32_nc3", "nonic", desc, config, trace, public_inputs, {"trace_seed": NONIC_SEED}


FIXTURES = {"fibonacci": fibonacci, "nonic": nonic}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("fixture", nargs="?", default="fibonacci", choices=sorted(FIXTURES))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    stem, air, desc, config, trace, public_inputs, extra = FIXTURES[args.fixture]()
    stark = p.Stark(desc, config, NUM_ROWS.bit_length() - 1)
    proof = stark.prove(trace, public_inputs)
    ok, why, _ = stark.verify(proof)
    assert ok, why
    params = stark.params
    words = lambda off: [int.from_bytes(proof[off + 8 * i:off + 8 * i + 8], "little") for i in range(4)]      # noqa: E731
    cap_bytes = 32 << params.cap_height
    meta = {
        "air": air, "num_rows": NUM_ROWS, "public_inputs": public_inputs, "num_challenges": config.num_challenges, "hasher": "poseidon",
        "params": {"degree_bits": params.degree_bits, "rate_bits": params.rate_bits, "cap_height": params.cap_height,
                   "proof_of_work_bits": params.proof_of_work_bits, "num_query_rounds": params.num_query_rounds,
                   "reduction_arity_bits": params.reduction_arity_bits},
        "num_bytes": len(proof),
        "trace_cap_first_words": words(0), "permutation_zs_cap_first_words": words(cap_bytes), "quotient_polys_cap_first_words": words(2 * cap_bytes),
    }
    meta.update(extra)
    with open(os.path.join(args.out, stem + ".bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(args.out, stem + ".json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%s: %d bytes, public inputs %s" % (stem, len(proof), public_inputs))


if __name__ == "__main__":
    main()
