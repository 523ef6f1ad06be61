"""The Python-integer model of vanishing(x) / Z_H(x) (tests/vanishing_model.py) on its own evidence, before it judges a kernel
(tests/test_quotient_model.py).  CPU only.

Against the oracle's prover: on satisfying witnesses of circuits over ten gate types, the model's values on the LDE coset, taken through
coset_ifft, are the proof's quotient chunks word for word.  Only the transforms (pinned elsewhere) and the inputs come from the oracle.
The four extension-field gates, which the oracle does not have: every constraint vanishes on the rows of tests/ext_gate_circuits.py's
witnesses and answers to its tampered cell."""
import numpy as np
import pytest

import ext_gate_circuits as egc
import vanishing_model as vm
from oracle_lib import rand_field
from proof_parser import ParsedProof
from transcript import poseidon_challenger, replay_transcript

P = vm.P


def oracle_inputs(orc, oc, w):
    """-> (desc, the three value batches, pi_hash, betas, gammas, alphas, deltas or None, the proof) of the oracle's proof of `w`"""
    op = w.prove(threads=4)
    d, ch = oc.product_desc(), op.challenges()
    # the lookup challenges are not in challenges(): the replay of the proof's transcript draws them
    replayed, _, _, deltas = replay_transcript(d, poseidon_challenger(orc), oc.digest, ch["public_inputs_hash"], ParsedProof(d, op.to_bytes()))
    assert replayed == ch
    return d, (oc.constants_sigmas(), w.wires(), op.zs_partial_products()), ch["public_inputs_hash"], ch["betas"], ch["gammas"], ch["alphas"], deltas, op


def _matmul(orc, m):
    oc = orc.circuit(m, threads=4)
    return oc, oc.witness(rand_field(3, m * m) % (2**32 - 1), rand_field(4, m * m) % (2**32 - 1), filler_seed=5)


def _kind(orc, kind, param, inputs):
    oc = orc.circuit_of_kind(kind, param, threads=4)
    return oc, oc.witness(np.array(inputs, dtype=np.uint64), np.zeros(0, dtype=np.uint64), filler_seed=param)


def _merkle(orc, height, index):
    from test_verifier import merkle_proof_circuit_inputs
    return _kind(orc, 14, height, merkle_proof_circuit_inputs(orc, height, index)[0])


def _random_access(orc, bits):
    v = rand_field(bits, (1 << bits,))
    return _kind(orc, 16, bits, np.concatenate([v, np.array([0, (1 << bits) - 1, 5 % (1 << bits)], dtype=np.uint64)]))


@pytest.mark.parametrize("name,build", [
    ("matmul m = 1", lambda orc: _matmul(orc, 1)),
    ("matmul m = 2", lambda orc: _matmul(orc, 2)),
    ("kind 15: eleven gate types, three selector groups, two lookup tables", lambda orc: _kind(orc, 15, 1, [0, 0])),
    ("kind 16: RandomAccessGate, 3 bits", lambda orc: _random_access(orc, 3)),
    ("kind 14: Merkle proof, swapped PoseidonGates", lambda orc: _merkle(orc, 3, 5)),
])
def test_the_model_reproduces_the_oracle_quotient_chunks(orc, name, build):
    oc, w = build(orc)
    d, values, pi_hash, betas, gammas, alphas, deltas, op = oracle_inputs(orc, oc, w)
    n = 1 << d.degree_bits
    cs, wires, zs = (orc.lde(orc.ifft(v), 3) for v in values)
    got = vm.vanishing_over_z_h(d, cs, wires, zs, pi_hash, betas, gammas, alphas, deltas)
    chunks = orc.coset_ifft(np.array(got, dtype=np.uint64), 7).reshape(16, n)
    assert (chunks == op.quotient_chunks()).all(), name
    if "Merkle" in name:
        swaps = {int(values[1][24][r]) for r, g in enumerate(oc.row_gates()) if g == vm.POSEIDON}      # PoseidonGate::WIRE_SWAP = 24
        assert swaps == {0, 1}


# ------------------------------------------------------------------------------- the four extension-field gates
EXT_GATES = [egc.ARITHMETIC_EXT, egc.MUL_EXT, egc.REDUCING, egc.REDUCING_EXT]


def _rows(circuit, gate):
    return [(consts, wires) for g, consts, wires in circuit.rows if g == gate]


@pytest.mark.parametrize("gate", EXT_GATES)
def test_extension_gate_constraints_vanish_on_the_witness_and_answer_to_a_tampered_cell(gate):
    constraints = vm.gate_constraints(gate)
    rows = _rows(egc.isolated([gate], seed=gate, rows_per_gate=3), gate) + _rows(egc.Chained(seed=2).circuit, gate)
    assert len(rows) >= 4
    nc = egc.NUM_CONSTRAINTS[gate]
    for consts, wires in rows:
        assert constraints(consts, wires, [0] * 4) == [0] * nc
    consts, wires = rows[-1]
    for j in range(nc):
        bad = list(wires)
        bad[egc.constraint_cell(gate, j)] = (bad[egc.constraint_cell(gate, j)] + 1) % P
        nonzero = {k for k, v in enumerate(constraints(consts, bad, [0] * 4)) if v}
        assert j in nonzero
        # an output, or the ReducingGate's base-field coefficient, feeds one constraint; an accumulator that is not the last one is also
        # the next step's operand
        step = j // 2
        alone = gate in (egc.ARITHMETIC_EXT, egc.MUL_EXT) or (gate == egc.REDUCING and j % 2 == 0) or step == nc // 2 - 1
        assert nonzero == {j} if alone else nonzero <= {j, 2 * step + 2, 2 * step + 3}


def test_filters_single_out_the_row_gate_on_the_chained_circuit():
    # gate.rs:277-284 on the selector columns of selectors.rs:111-170: at every trace row the row's gate has a non-zero filter, every
    # other gate a zero one, and the row's own constraints vanish
    c = egc.Chained(seed=3).circuit
    d = vm.Shape(c.desc)
    assert c.desc.num_selectors == 2 and c.desc.num_gates == 8
    for r, (gate, consts, wires) in enumerate(c.rows):
        col = [int(c.constants[k, r]) for k in range(c.desc.num_constants)]
        assert col[c.desc.num_selectors:] == consts
        for g, (constraints, selector_index, start, end) in enumerate(d.gates):
            f = vm.gate_filter(g, start, end, col[selector_index], True)
            assert (f != 0) == (c.desc.gate_types[g] == gate)
            if f:
                assert not any(constraints(consts, wires, [0] * 4))
