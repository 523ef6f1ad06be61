#!/usr/bin/env python3
"""Writes the committed MemoryStark proof, tests/golden/memory_stark_n32.bin / .json (run on the GPU): the log of
tests/memory_cases.py end_to_end_log(5) -- 22 memory operations whose trace has 2^5 rows, four of them pushed by fill_gaps and six
padding copies in the middle of the trace -- sorted, counted and filled on the device (gl_memory_trace_*), proved from there
(gl_stark_prove_device) under StarkConfig::standard_fast_config against the description gl_memory_stark_desc exports.  The CPU test
tests/test_memory_model.py verifies it with the host verifier and tampers with it.

--out DIR writes there instead of tests/golden."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plonky2_demo_amd as p  # noqa: E402

LG_ROWS = 5


def main():
    import memory_cases as mc
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    log = mc.end_to_end_log(LG_ROWS)
    ops = mc.records(log)
    ctx = p.default_context()
    trace = p.MemoryTrace(ops, ctx=ctx)
    assert trace.rows == 1 << LG_ROWS
    config = p.StarkConfig.standard_fast_config()
    stark = p.Stark(p.memory_stark(), config, LG_ROWS, ctx=ctx)
    d = ctx.alloc(26 * trace.rows * 8)
    trace.fill(d.ptr)
    proof = stark.prove_device(d.ptr, [])
    assert (d.download((26, trace.rows)) == p.memory_trace_host(ops)).all(), "the device and the host disagree"
    ok, why, _ = stark.verify(proof)
    assert ok, why
    params = stark.params
    meta = {
        "air": "memory", "num_rows": trace.rows, "num_challenges": config.num_challenges, "hasher": "poseidon",
        "params": {"degree_bits": params.degree_bits, "rate_bits": params.rate_bits, "cap_height": params.cap_height,
                   "proof_of_work_bits": params.proof_of_work_bits, "num_query_rounds": params.num_query_rounds,
                   "reduction_arity_bits": params.reduction_arity_bits},
        "num_bytes": len(proof),
        "ops_fields": ["filter", "is_read", "context", "segment", "virt", "timestamp", "value limbs"],
        "ops": [[o["filter"], o["is_read"], o["context"], o["segment"], o["virt"], o["timestamp"], o["value"]] for o in log],
    }
    with open(os.path.join(args.out, "memory_stark_n32.bin"), "wb") as f:
        f.write(proof)
    with open(os.path.join(args.out, "memory_stark_n32.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")
    print("memory_stark_n32: %d bytes, %d ops, %d rows" % (len(proof), len(log), trace.rows))


if __name__ == "__main__":
    main()
