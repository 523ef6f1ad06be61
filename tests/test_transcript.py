"""The shared transcript helpers (tests/transcript.py, tests/proof_parser.py) on their own evidence, before they drive the phase-level
ABI on the GPU.  CPU only: the library's Challenger is host code, the proofs are the oracle's and the stored one."""
import os

import numpy as np
import pytest

from ext_gate_circuits import isolated, ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT
from oracle_lib import P, rand_field
from proof_parser import ParsedProof, proof_bytes
from transcript import poseidon_challenger, public_inputs_hash, replay_transcript

U64 = np.uint64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_poseidon_challenger_matches_the_model(orc):
    # observations that cross the rate or are empty, HashOuts of both kinds, more than 8 challenges in a row or none
    import plonky2_demo_amd as p
    ch, mo = p.Challenger(), poseidon_challenger(orc)
    rng = np.random.default_rng(11)
    pi_hash, cap = rand_field(12, 4), rand_field(13, (16, 4))
    assert ch.get_n_challenges(3) == mo.get(3)                       # a squeeze of the all-zero state
    for step in range(40):
        xs = rng.integers(0, 2**64, int(rng.integers(0, 14)), dtype=U64)
        ch.observe_elements(xs); mo.observe(xs)
        if step % 5 == 1:
            ch.observe_hashes(pi_hash, hasher="poseidon"); mo.observe_hashes(pi_hash, inner=True)
        if step % 7 == 2:
            ch.observe_hashes(cap); mo.observe_hashes(cap)
        k = int(rng.integers(0, 11))
        assert ch.get_n_challenges(k) == mo.get(k)
        st, buf = ch.state()
        assert [int(x) % P for x in st] == [x % P for x in mo.state] and [int(x) % P for x in buf] == mo.inp


@pytest.fixture(scope="module")
def oracle_proofs(orc):
    """(desc, circuit digest, public inputs, the oracle's proof) of matmul m = 2 and of the n = 32 lookup circuit"""
    mm = orc.circuit(2, threads=4)
    lk = orc.circuit_of_kind(8, 50, threads=4)
    ws = {"matmul": mm.witness(rand_field(3, 4) % (2**32 - 1), rand_field(4, 4) % (2**32 - 1), filler_seed=5),
          "lookup": lk.witness(np.arange(3, 53, dtype=U64), np.zeros(0, dtype=U64), filler_seed=9)}
    return {name: (oc.product_desc(), oc.digest, ws[name].public_inputs(), ws[name].prove(threads=4)) for name, oc in (("matmul", mm), ("lookup", lk))}


@pytest.mark.parametrize("name", ["matmul", "lookup"])
def test_replay_with_the_poseidon_model_reproduces_the_oracle_transcript(orc, oracle_proofs, name):
    d, digest, pis, op = oracle_proofs[name]
    assert d.degree_bits == 5 or name == "matmul"
    chal, response, x_index, deltas = replay_transcript(d, poseidon_challenger(orc), digest, public_inputs_hash(orc, pis), ParsedProof(d, op.to_bytes()))
    assert chal == op.challenges()
    assert response >> (64 - d.proof_of_work_bits) == 0
    assert x_index == op.query_indices()
    if name == "lookup":
        assert len(deltas) == 8 and deltas[:4] == chal["betas"] + chal["gammas"]
    else:
        assert deltas is None


def _rewritten(d, by):
    pp = ParsedProof(d, by)
    return proof_bytes(d, pp.caps, pp.openings, pp.fri_caps, pp.queries, pp.final_poly, pp.pow_witness, pp.public_inputs)


@pytest.mark.parametrize("name", ["matmul", "lookup"])
def test_the_writer_inverts_the_parser_on_the_oracle_proofs(oracle_proofs, name):
    d, _, _, op = oracle_proofs[name]
    assert _rewritten(d, op.to_bytes()) == op.to_bytes()


def test_the_writer_inverts_the_parser_on_the_stored_proof():
    d = isolated([ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT], 77, rows_per_gate=1).desc
    with open(os.path.join(GOLDEN, "ext_gates_n8_proof.bin"), "rb") as f:
        by = f.read()
    assert _rewritten(d, by) == by
