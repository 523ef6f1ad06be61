#!/usr/bin/env python3
"""Writes tests/golden/stark_ctl_set.bin / .json (run on the GPU): the set proof of the three-table system of tests/stark_ctl_airs.py at
2^5 / 2^6 / 2^5 rows, num_challenges 2, Poseidon, which the CPU tests verify and tamper with (tests/test_stark_ctl_host.py) and the GPU
test holds current (tests/test_stark_ctl.py).  The description is tests/stark_ctl_airs.py's and the traces are its traces(lgs, seed): the
json records what to call them with."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402
import stark_ctl_airs as airs  # noqa: E402

LGS, NC, SEED = [5, 6, 5], 2, 5


def make():
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, LGS, airs.config(p, NC)))
    proof = sset.prove(airs.traces(LGS, seed=SEED))
    ok, why, _, _ = sset.verify(proof)
    assert ok, why
    params = sset.desc.fri_params(0)
    meta = {"system": "tests/stark_ctl_airs.py TABLES, LOOKUPS", "degree_bits": LGS, "num_challenges": NC, "trace_seed": SEED, "hasher": "poseidon",
            "config": {"rate_bits": params.rate_bits, "cap_height": params.cap_height, "proof_of_work_bits": params.proof_of_work_bits,
                       "num_query_rounds": params.num_query_rounds},
            "num_ctl_zs": [c[1] for c in sset.counts], "num_permutation_zs": [c[0] for c in sset.counts], "num_bytes": len(proof)}
    return proof, meta


def main():
    proof, meta = make()
    golden = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(golden, "stark_ctl_set.bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(golden, "stark_ctl_set.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("%d bytes" % len(proof))


if __name__ == "__main__":
    main()
