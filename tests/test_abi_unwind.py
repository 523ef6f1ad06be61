"""include/plonky2_mi355x.h promises that no entry point unwinds.  The host-only entry points (host_api.hip, verifier.hip,
serialization.hip), the context's (context.hip, over the stub HIP runtime) and the pools' lane runner (lanes.hpp) are rebuilt with
-fsanitize=address,undefined into a stand-alone program whose operator new fails at the k-th allocation, for EVERY k of every listed
call (tools/sanitizer/abi_unwind.cpp): each failure must come back as a status with a text and null out-handles, the call must give
its first result again afterwards, and nothing may leak.  CPU only."""
import os
import re
import subprocess

import numpy as np

from oracle_lib import rand_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tools", "sanitizer")

# every call the harness lists, and whether it allocates at all
CALLS = [
    ("gl_matmul_circuit_build_h(m=2, zero_knowledge=0, hasher=0)", True),
    ("gl_matmul_circuit_build_h(m=2, zero_knowledge=0, hasher=1)", True),
    ("gl_matmul_circuit_build_h(m=2, zero_knowledge=1, hasher=0)", True),
    ("gl_matmul_circuit_build_h(m=2, zero_knowledge=1, hasher=1)", True),
    ("gl_host_circuit_constants_sigmas", True),
    ("gl_host_circuit_wire_classes", False),
    ("gl_matmul_witness", True),
    ("gl_challenger_new_h(0) + observe + get_challenges + state", True),
    ("gl_challenger_new_h(1) + observe + get_challenges + state", True),
    ("gl_verify", True),
    ("gl_host_circuit_verify", True),
    ("gl_common_data_to_bytes", True),
    ("gl_common_data_from_bytes", False),
    ("gl_verifier_only_to_bytes_h", True),
    ("gl_verifier_only_from_bytes_h", False),
    ("gl_verify_bytes", True),
    ("context: gl_ctx_create + gl_ctx_destroy", True),
    ("context: gl_dev_alloc + gl_copy_h2d + gl_copy_d2h + gl_ctx_synchronize", True),
    ("context: gl_ctx_timing_report", True),
    ("context: gl_ctx::pool_alloc", True),
    ("lanes: thread start", True),
]


def test_every_failing_allocation_comes_back_as_a_status(orc, tmp_path):
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    m = 2
    hc, oc = p.MatmulCircuit(m), orc.circuit(m, threads=2)
    a, b = rand_field(40 + m, m * m) % (2**32 - 1), rand_field(41 + m, m * m) % (2**32 - 1)
    cap, dig = np.ascontiguousarray(oc.constants_sigmas_cap), np.ascontiguousarray(oc.digest)
    (tmp_path / "desc.bin").write_bytes(bytes(hc.desc))
    (tmp_path / "cap.bin").write_bytes(cap.tobytes())
    (tmp_path / "dig.bin").write_bytes(dig.tobytes())
    (tmp_path / "proof.bin").write_bytes(oc.witness(a, b, filler_seed=0).prove(threads=2).to_bytes())
    (tmp_path / "vd.bin").write_bytes(api.verifier_data_to_bytes(hc.desc, cap, dig))
    subprocess.check_call(["make", "-s", "-C", SAN, "abi_unwind"])
    r = subprocess.run([os.path.join(SAN, "abi_unwind"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    for name, allocates in CALLS:
        mo = re.search(r"^%s: (\d+) allocations, (\d+) failed cleanly$" % re.escape(name), r.stdout, re.M)
        assert mo, "%s is missing from the harness's output:\n%s" % (name, r.stdout)
        assert mo.group(1) == mo.group(2), mo.group(0)
        assert int(mo.group(1)) >= 1 or not allocates, mo.group(0)
    assert "lanes: std::bad_alloc thrown on lane 0 and on lane 2 became GL_ERR_INTERNAL" in r.stdout
    assert "lanes: std::runtime_error became GL_ERR_INTERNAL" in r.stdout
    assert "lanes: the first error came back with its own text and stopped its lane" in r.stdout
    assert "the failing one gave the block back" in r.stdout
    for needle in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert needle not in r.stderr, r.stderr[-3000:]
