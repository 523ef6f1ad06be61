"""The committed zero-knowledge proof (tests/golden/zk_matmul2_n256.bin, made on the GPU by tools/make_zk_fixture.py) on machines without
one: the integer derivation of tests/zk_model.py gives the same bytes from the inputs recorded beside it, gl_verify accepts them, and
gl_verify and the model verifier reject the same tampered copies with the same named check.  A change to the zero-knowledge path that
alters a proof's bytes is seen here first; a change to the model that alters them is seen here too."""
import ctypes
import json
import os

import numpy as np
import pytest

import fri_openings_model as fm
import zk_circuits as zc
import zk_model as zm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STEM = "zk_matmul2_n256"
GL_ERR_VERIFY = 6


@pytest.fixture(scope="module")
def case(orc):
    """(description, public inputs, the committed bytes, the model's derivation), made once and left unchanged"""
    import plonky2_demo_amd as p
    with open(os.path.join(GOLDEN, STEM + ".json")) as f:
        j = json.load(f)
    with open(os.path.join(GOLDEN, STEM + ".bin"), "rb") as f:
        proof = f.read()
    assert j["circuit"] == "matmul" and j["num_bytes"] == len(proof)
    a, b = np.array(j["a"], dtype=np.uint64), np.array(j["b"], dtype=np.uint64)
    desc, cs, wires, pis, g = zc.plain_matmul(p, j["m"], a, b, j["filler_seed"])
    zd, cs2, wires2 = zc.embed_zk(desc, cs, wires, g, j["num_query_rounds"], j["proof_of_work_bits"], j["hasher"])
    assert (zd.degree_bits, zd.num_gate_rows, zd.num_fri_rounds) == (j["degree_bits"], j["num_gate_rows"], j["num_fri_rounds"]) == (8, 6, 1)
    model = zm.derive(orc, zm.hashing_of(orc, j["hasher"]), zd, cs2, wires2, pis, bytes.fromhex(j["salt_seed"]))
    return p, j, zd, pis, proof, model


def library_verdict(p, d, m, by):
    """(accepted, message) of gl_verify (host code) under the model's constants || sigmas cap and circuit digest"""
    from plonky2_demo_amd._lib import lib
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    cap, digest, buf = np.ascontiguousarray(m.cs_cap, dtype=np.uint64), np.ascontiguousarray(m.digest, dtype=np.uint64), np.frombuffer(by, dtype=np.uint8)
    st = lib.gl_verify(ctypes.byref(d), vp(cap), vp(digest), vp(buf), buf.size)
    assert st in (0, GL_ERR_VERIFY), st
    return st == 0, "" if st == 0 else lib.gl_last_error().decode()


def test_the_fixture_is_the_shared_case(case):
    p, j, d, pis, proof, m = case
    (_, mm, operand_seed, filler_seed), hasher, queries, pow_bits, seed, n, rounds = zc.CASES[zc.FIXTURE_CASE]
    a, b = zc.matmul_operands(mm, operand_seed)
    assert (j["m"], j["a"], j["b"], j["filler_seed"]) == (mm, [int(v) for v in a], [int(v) for v in b], filler_seed)
    assert (j["hasher"], j["num_query_rounds"], j["proof_of_work_bits"], j["salt_seed"], 1 << j["degree_bits"]) == (hasher, queries, pow_bits, seed.hex(), n)
    assert len(proof) < 32 * 1024


def test_model_bytes_equal_the_committed_proof(case):
    p, j, d, pis, proof, m = case
    assert m.z_after_gate_rows == [1, 1] and m.z_after_pairs == [1, 1] and m.z_on_blinding_rows_is_one and not m.quotient_sampled
    why = zm.describe_difference(d, proof, m)
    assert why is None, why
    assert proof == m.bytes


def test_gl_verify_and_the_model_verifier_accept_the_committed_proof(case, orc):
    p, j, d, pis, proof, m = case
    assert library_verdict(p, d, m, proof) == (True, "")
    trace = {}
    assert zm.verify(orc, m.hashing, d, m.cs_cap, m.digest, proof, pis, trace=trace) == fm.ACCEPTED
    assert trace["x_indices"] == m.x_index and trace["pow_response"] == m.pow_response


# (name, the byte to flip given the layout and the query index, the check that has to name it; None: whichever the model names -- a word inside
# the FRI transcript moves the proof-of-work response, which fails 255 times in 256 and lets a later check fail otherwise)
def _x(m):
    return m.x_index[0]


TAMPER = (
    [("cap of oracle %d" % (k + 1), lambda lay, m, k=k: lay.caps[k] + 32 * 5 + 8, fm.VANISHING) for k in range(3)]
    + [("opening group %s" % name, lambda lay, m, name=name: lay.openings[name] + 16 + 8 * (len(name) % 2), fm.VANISHING)
       for name in ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "quotient")]
    + [("FRI commit cap", lambda lay, m: lay.fri_caps[0] + 32 * 9, None),
       ("final polynomial", lambda lay, m: lay.final + 8 * 7, None),
       ("PoW witness", lambda lay, m: lay.pow, fm.POW)]
    + [("leaf value of oracle %d" % o, lambda lay, m, o=o: lay.leaf[0][o] + 8 * 2, fm.INITIAL_MERKLE) for o in range(4)]
    + [("salt word %d of oracle %d" % (w, o), lambda lay, m, o=o, w=w: lay.leaf[0][o] + 8 * (lay.leaf_len[o] - 4 + w), fm.INITIAL_MERKLE)
       for o, w in ((1, 0), (2, 3), (3, 1))]
    + [("initial sibling", lambda lay, m: lay.sibling[0][2] + 32 * 3 + 8, fm.INITIAL_MERKLE),
       ("evals[x & 15] of the step", lambda lay, m: lay.step_evals[0][0] + 16 * (_x(m) & 15), fm.FRI_CONSISTENCY),
       ("another eval of the step leaf", lambda lay, m: lay.step_evals[0][0] + 16 * ((_x(m) + 5) & 15) + 8, fm.STEP_MERKLE),
       ("step sibling", lambda lay, m: lay.step_sibling[0][0] + 32 + 16, fm.STEP_MERKLE)])


@pytest.mark.parametrize("name,where,code", TAMPER, ids=[t[0] for t in TAMPER])
def test_tampering_is_rejected_by_both_verifiers_with_the_same_check(case, orc, name, where, code):
    p, j, d, pis, proof, m = case
    lay = zm.layout(d, len(pis))
    assert lay.end == len(proof) and lay.leaf_len == [84, 139, 24, 20]
    at = where(lay, m)
    assert 0 <= at < lay.pow + 8
    bad = zm.flip(proof, at, bit=3)
    want = zm.verify(orc, m.hashing, d, m.cs_cap, m.digest, bad, pis)
    assert want != fm.ACCEPTED and (code is None or want == code), (name, want)
    ok, why = library_verdict(p, d, m, bad)
    assert not ok and why.startswith(p.api.verify_check_message(want)), (name, want, why)
