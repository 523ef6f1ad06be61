"""Seeded zero-knowledge proofs, byte for byte against the integer derivation of tests/zk_model.py.

The CPU oracle cannot build a zero-knowledge circuit and the phase API refuses one, so until here a zk proof was judged only by the
library's own verifier, which shares the transcript, the shape code and the notion of "unsalted prefix" with the prover.  Each case below
proves once on the device (gl_witness_blind, then gl_prove_device_seeded, one seed for both) and derives the same proof from plain
integers: blinded wires, salted caps, Z and partial products over the blinding rows, the quotient, the openings, the FRI commit phase, the
smallest PoW witness, the query rounds with their salted leaves.  The circuits are small because num_query_rounds is small
(zk_circuits.CASES): n = 256, 512 and 1024, one and two reduction rounds, Poseidon and Keccak.
  A  the captured intermediates column by column, then the bytes; the first differing section is named
  B  an independent verdict: zk_model.verify accepts, and names the check the library names after a flipped salt word / opened value
  C  the edge witness
  D  the standard size (n = 2^14, 28 queries), where the cost is proportional to the queries
  E  a ProverPool proof (OS entropy: not re-derivable) under the independent verdict
At n = 256 and 512 the model derives the quotient chunks from all 8 n LDE points (2.5 and 5.5 s of one CPU core); at n = 1024 that alone
takes 13 to 18 s and the case 20 to 26 s, so there the prover's chunks are compared with the model's vanishing(x) / Z_H(x) at the 64+ points
of zk_model.quotient_points and the derivation goes on from them (8 s).
"""
import numpy as np
import pytest

import fri_openings_model as fm
import zk_circuits as zc
import zk_model as zm
from oracle_lib import P
from proof_parser import ParsedProof
from transcript import FRI_OPENINGS, public_inputs_hash, replay_transcript

pytestmark = pytest.mark.gpu
U64 = np.uint64
FULL_QUOTIENT_UP_TO = 512
QUOTIENT_COLUMNS = ["quotient chunk %d of challenge %d" % (k, b) for b in range(2) for k in range(8)]
_cases = {}


def proven(gpu, orc, name):
    """one proof and one model derivation per case, made once and left unchanged"""
    if name not in _cases:
        p, ctx = gpu
        zd, cs, wires, pis, seed = zc.build_case(p, orc, name)
        cd = p.GenericCircuitData(zd, cs, ctx=ctx)
        buf = ctx.alloc(wires.nbytes)
        buf.upload(wires)
        cd.blind_witness(buf.ptr, seed=seed)
        blinded = buf.download(wires.shape)
        proof = cd.prove_device(buf.ptr, pis, seed=seed)
        buf.free()
        sampled = (1 << zd.degree_bits) > FULL_QUOTIENT_UP_TO
        model = zm.derive(orc, zm.hashing_of(orc, zd.hasher), zd, cs, wires, pis, seed, quotient_chunks=proof.quotient_chunks() if sampled else None)
        print("%s: model %.1f s (%s)" % (name, sum(model.times.values()), ", ".join("%s %.1f" % kv for kv in model.times.items())))
        _cases[name] = (cd, zd, pis, blinded, proof, proof.to_bytes(), model)
    return _cases[name]


# ------------------------------------------------------------------------------- A: every byte
def cap_difference(oracle, got, want):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=1))
    return "cap of the %s oracle: %d of %d hashes differ, first cap entry %d" % (zm.ORACLE_NAMES[oracle], len(bad), len(want), bad[0])


@pytest.mark.parametrize("name", list(zc.CASES))
def test_zk_proof_equals_the_model(gpu, orc, name):
    cd, d, pis, blinded, proof, by, m = proven(gpu, orc, name)
    g = d.num_gate_rows
    assert (blinded == m.blinded).all(), zm.columns_difference("blinded wires", ["wire %d" % w for w in range(135)], blinded, m.blinded)
    # what the row pairs are for: Z is back at 1 behind the gate rows and behind the last pair (every blinding row's sigma is the identity)
    assert m.z_after_gate_rows == [1, 1] and m.z_after_pairs == [1, 1] and m.z_on_blinding_rows_is_one
    assert g + m.regular + 2 * m.pairs <= 1 << d.degree_bits
    assert (cd.constants_sigmas_cap == m.cs_cap).all() and (cd.circuit_digest == m.digest).all()
    # in the transcript's order, so that what is named is the first thing that went wrong: a cap moves every challenge behind it
    caps = proof.caps()
    assert (caps[0] == m.caps[0]).all(), cap_difference(1, caps[0], m.caps[0])
    why = zm.columns_difference("Z and partial products", zm.ZS_COLUMNS, proof.zs_partial_products(), m.zs)
    assert why is None, why
    assert (caps[1] == m.caps[1]).all(), cap_difference(2, caps[1], m.caps[1])
    if m.quotient_sampled:
        bad = [(i, b) for i in m.points for b in range(2) if m.quotient_given[i][b] != m.quotient_model[i][b]]
        assert len(m.points) >= 64 and not bad, "quotient: t(x) of the prover's chunks differs from vanishing / Z_H at %d of %d points, first LDE point %d, challenge %d: %d, model %d" % (
            len(bad), 2 * len(m.points), bad[0][0], bad[0][1], m.quotient_given[bad[0][0]][bad[0][1]], m.quotient_model[bad[0][0]][bad[0][1]])
    else:
        why = zm.columns_difference("quotient chunks", QUOTIENT_COLUMNS, proof.quotient_chunks(), m.chunks)
        assert why is None, why
    assert (caps[2] == m.caps[2]).all(), cap_difference(3, caps[2], m.caps[2])
    why = zm.describe_difference(d, by, m)
    assert why is None, why
    assert by == m.bytes
    assert proof.query_indices() == m.x_index and proof.challenges()["pow_witness"] == m.pow_witness


def test_committed_fixture_is_current(gpu, orc):
    # tests/golden/zk_matmul2_n256.bin (tools/make_zk_fixture.py), which tests/test_zk_model_host.py derives again without a GPU
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zk_matmul2_n256.bin"), "rb") as f:
        committed = f.read()
    assert proven(gpu, orc, zc.FIXTURE_CASE)[5] == committed


# ------------------------------------------------------------------------------- B: an independent verdict
def verdicts(p, orc, cd, d, hashing, by, pis):
    """(the model's GL_CHECK_* code, the library's (accepted, message))"""
    return zm.verify(orc, hashing, d, cd.constants_sigmas_cap, cd.circuit_digest, by, pis), cd.verify(by)


def assert_same_verdict(p, code, got, want_code=None):
    ok, why = got
    assert ok == (code == fm.ACCEPTED)
    assert why == "" if ok else why.startswith(p.api.verify_check_message(code)), (code, why)
    if want_code is not None:
        assert code == want_code, (code, why)


@pytest.mark.parametrize("name", list(zc.CASES))
def test_model_verifier_and_library_give_the_same_verdicts(gpu, orc, name):
    p, ctx = gpu
    cd, d, pis, blinded, proof, by, m = proven(gpu, orc, name)
    lay = zm.layout(d, len(pis))
    assert lay.end == len(by) and lay.leaf_len == [d.num_constants + 80, 139, 24, 20]
    assert_same_verdict(p, *verdicts(p, orc, cd, d, m.hashing, by, pis), want_code=fm.ACCEPTED)
    last = d.num_query_rounds - 1
    # one salt word of a queried leaf, in each blinded tree: outside the transcript, so the initial Merkle proof is what fails
    for o, q, word in ((1, 0, 135), (2, last, 20 + 3), (3, 0, 16 + 1)):
        bad = zm.flip(by, lay.leaf[q][o] + 8 * word, bit=5)
        assert_same_verdict(p, *verdicts(p, orc, cd, d, m.hashing, bad, pis), want_code=fm.INITIAL_MERKLE)
    # one opened value: the identity at zeta no longer holds (the transcript up to zeta does not read the openings)
    for group, column in (("wires", 134), ("zs_next", 1), ("quotient", 15)):
        bad = zm.flip(by, lay.openings[group] + 16 * column + 8, bit=2)
        assert_same_verdict(p, *verdicts(p, orc, cd, d, m.hashing, bad, pis), want_code=fm.VANISHING)
    # the last leaf word in front of the salt, a sibling, the final polynomial: rejected where the model says
    for bad in (zm.flip(by, lay.leaf[last][1] + 8 * 134), zm.flip(by, lay.sibling[0][3] + 3), zm.flip(by, lay.final + 8, bit=7)):
        code, got = verdicts(p, orc, cd, d, m.hashing, bad, pis)
        assert code != fm.ACCEPTED
        assert_same_verdict(p, code, got)


# ------------------------------------------------------------------------------- C: the edge witness
def test_edge_witness_and_its_blinding_stream(gpu, orc):
    p, ctx = gpu
    name = "matmul2-edges-q1"
    cd, d, pis, blinded, proof, by, m = proven(gpu, orc, name)
    a, b = zc.matmul_operands(2, "edges")
    assert {0, 1, zc.MAX_OPERAND} <= set(int(v) for v in a) and {0, 1, zc.MAX_OPERAND} <= set(int(v) for v in b)
    # the public inputs are (a_ij, b_ij, c_ij) entry by entry; the product holds 0, 1 and the largest operand's square, which is above 2^63
    product = [sum(int(a[2 * i + k]) * int(b[2 * k + j]) for k in range(2)) % P for i in range(2) for j in range(2)]
    assert [int(v) for v in pis] == [int(v) for t in zip(a, b, product) for v in t]
    assert {0, 1, zc.MAX_OPERAND**2 % P} <= set(product) and zc.MAX_OPERAND**2 % P > 2**63
    # the blinding stream of this seed, by the model: spread over the whole field, nothing repeated, both halves of the u64 range present
    g = d.num_gate_rows
    rows = m.blinded[:, g:g + m.regular].reshape(-1)
    assert len(set(rows.tolist())) == rows.size and int(rows.min()) < P >> 10 and int(rows.max()) > P - (P >> 10)
    assert ((rows >> U64(63)) == 1).mean() > 0.4 and ((rows >> U64(63)) == 0).mean() > 0.4
    assert (blinded == m.blinded).all() and by == m.bytes


# ------------------------------------------------------------------------------- D: the standard size
def transcript_before_the_witness(d, ch, digest, pi_hash, pp):
    """replay_transcript up to the final polynomial: the challenger as fri_proof_of_work finds it"""
    ch.observe_hashes(digest)
    ch.observe_hashes(pi_hash, inner=True)
    for cap in pp.caps:
        ch.observe_hashes(cap)
        ch.get(4 if cap is pp.caps[0] else 2)
    for name in FRI_OPENINGS:
        ch.observe(pp.openings[name])
    ch.get(2)
    for cap in pp.fri_caps:
        ch.observe_hashes(cap)
        ch.get(2)
    ch.observe(pp.final_poly)
    return ch


def test_standard_size_queries_carry_the_model_salt(gpu, orc):
    p, ctx = gpu
    m2, seed = 2, zc.SEED
    hc = p.MatmulCircuit(m2, zero_knowledge=True)
    cd = hc.build(ctx)
    d = hc.desc
    assert (d.degree_bits, d.num_query_rounds, d.proof_of_work_bits, d.num_fri_rounds) == (14, 28, 16, 3)
    wires, pis = hc.witness(*zc.matmul_operands(m2, 3), filler_seed=5)
    buf = ctx.alloc(wires.nbytes)
    buf.upload(wires)
    cd.blind_witness(buf.ptr, seed=seed)
    blinded = buf.download(wires.shape)
    proof = cd.prove_device(buf.ptr, pis, seed=seed)
    buf.free()
    want = zc.model_blinded_wires(wires, d.num_gate_rows, seed)
    assert (blinded == want).all(), zm.columns_difference("blinded wires", ["wire %d" % w for w in range(135)], blinded, want)
    by = proof.to_bytes()
    pp = ParsedProof(d, by)
    H = zm.PoseidonHashing(orc)
    pi_hash = public_inputs_hash(orc, pis)
    # the transcript on the model challenger
    chal, response, x_index, _ = replay_transcript(d, H.challenger(), cd.circuit_digest, pi_hash, pp)
    assert chal == proof.challenges() and x_index == proof.query_indices()
    assert response >> (64 - d.proof_of_work_bits) == 0
    # the witness is the smallest
    ch = transcript_before_the_witness(d, H.challenger(), cd.circuit_digest, pi_hash, pp)
    state = list(ch.state)
    state[:len(ch.inp)] = ch.inp
    valid = []
    for base in range(0, pp.pow_witness + 1, 1 << 14):
        cand = np.arange(base, min(base + (1 << 14), pp.pow_witness + 1), dtype=U64)
        valid += [int(c) for c in cand[H.pow_valid(state, len(ch.inp), cand, d.proof_of_work_bits)]]
    assert valid == [pp.pow_witness]
    # every queried initial leaf is [oracle LDE row | model salt], every path leads to its cap
    lgN = d.degree_bits + d.rate_bits
    columns = [(hc.constants_sigmas(), True), (blinded, True), (proof.zs_partial_products(), True), (proof.quotient_chunks(), False)]
    batches = [orc.batch(cols, d.rate_bits, d.cap_height, from_values=fv, threads=8) for cols, fv in columns]
    caps = [cd.constants_sigmas_cap] + list(pp.caps)
    for q, (x, (init, steps)) in enumerate(zip(x_index, pp.queries)):
        row = int(format(x, "0%db" % lgN)[::-1], 2)                  # leaf x is LDE row bitrev(x); the salt's element index is the row
        for o in range(4):
            leaf, siblings = init[o]
            want = batches[o].get_leaf(x)
            if zm.ORACLE_BLINDING[o]:
                want = np.concatenate([want, [zc.model_elements(seed, zc.GL_STREAM_SALT + 4 * o + j, row, 1)[0] for j in range(4)]]).astype(U64)
            assert (leaf == want).all(), "query %d (index %d), %s oracle: leaf word %d" % (q, x, zm.ORACLE_NAMES[o], int(np.flatnonzero(leaf != want)[0]))
            assert H.verify_path(leaf, x, caps[o], siblings), "query %d (index %d), %s oracle: path" % (q, x, zm.ORACLE_NAMES[o])
        for r, (leaf, siblings) in enumerate(steps):
            x >>= d.fri_arity_bits[r]
            assert H.verify_path(leaf, x, pp.fri_caps[r], siblings), "query %d, FRI tree of round %d: path" % (q, r)


# ------------------------------------------------------------------------------- E: the pool
def test_pool_proof_under_the_independent_verdict(gpu, orc):
    p, _ = gpu
    hc = p.MatmulCircuit(2, zero_knowledge=True)
    a, b = zc.matmul_operands(2, 21)
    pool = p.ProverPool(hc, lanes=4)
    try:
        by = pool.prove_matmul([(a, b)], filler_seeds=[9])[0].to_bytes()
        cap, digest = pool.constants_sigmas_cap.copy(), pool.circuit_digest.copy()
    finally:
        pool.close()
    d, H = hc.desc, zm.PoseidonHashing(orc)
    lay = zm.layout(d, d.num_public_inputs)
    assert lay.end == len(by)
    assert zm.verify(orc, H, d, cap, digest, by) == fm.ACCEPTED and hc.verify(by, cap, digest) == (True, "")
    bad = zm.flip(by, lay.leaf[27][2] + 8 * 21)                      # a salt word of the last query's Z leaf
    ok, why = hc.verify(bad, cap, digest)
    assert zm.verify(orc, H, d, cap, digest, bad) == fm.INITIAL_MERKLE and not ok and why.startswith(p.api.verify_check_message(fm.INITIAL_MERKLE))
