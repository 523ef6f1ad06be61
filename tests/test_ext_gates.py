"""ArithmeticExtensionGate, MulExtensionGate, ReducingGate and ReducingExtensionGate (gate types 10..13): circuits built and witnessed by
the independent model of ext_gate_circuits.py, proved on the GPU, verified by gl_verify.  The CPU oracle has none of these gates, so
nothing here is byte parity with a Rust proof ("parity unpinned"): acceptance of the model's witnesses shows that the enforced
constraints vanish on the true relation, the per-constraint tampering that none is missing."""
import os
import threading

import numpy as np
import pytest

import ext_gate_circuits as egc
from ext_gate_circuits import ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT, P
from transcript import drive_phase_api, poseidon_challenger

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_GATES = [ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT]
NAMES = {ARITHMETIC_EXT: "arithmetic_ext", MUL_EXT: "mul_ext", REDUCING: "reducing", REDUCING_EXT: "reducing_ext"}
FIXTURE_SEED = 77


def _fixture_circuit():
    """the n = 8 circuit of the stored proof: one row of each of the four gates, isolated family"""
    return egc.isolated(NEW_GATES, FIXTURE_SEED, rows_per_gate=1)


def _build(p, c, ctx=None):
    return p.GenericCircuitData.from_classes(c.desc, c.constants, c.classes, ctx=ctx)


_NO_PIS = np.zeros(0, dtype=np.uint64)


# ------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("gate", NEW_GATES, ids=[NAMES[g] for g in NEW_GATES])
def test_each_gate_alone_proves_and_verifies(gpu, gate):
    p, ctx = gpu
    c = egc.isolated([gate], seed=10 + gate)
    assert c.n == 8 and [r[0] for r in c.rows[:2]] == [gate, gate]
    flat = [v for r in c.rows[:2] for v in r[2]] + [v for r in c.rows[:2] for v in r[1]]
    assert {0, 1, P - 1} <= set(flat)
    cd = _build(p, c, ctx)
    proof = cd.prove(c.wires(), _NO_PIS).to_bytes()
    assert cd.verify(proof) == (True, "")
    vd = p.api.verifier_data_to_bytes(cd.desc, cd.constants_sigmas_cap, cd.circuit_digest)
    assert p.api.verify_bytes(vd, proof) == (True, "")


@pytest.mark.gpu
@pytest.mark.parametrize("gate", NEW_GATES, ids=[NAMES[g] for g in NEW_GATES])
def test_every_constraint_rejects_a_witness_that_breaks_it(gpu, gate):
    # the gate rows' wires are in no copy constraint, so only the gate constraint can reject; constraint j is broken on gate row j mod 2
    p, ctx = gpu
    c = egc.isolated([gate], seed=20 + gate)
    cd = _build(p, c, ctx)
    good = c.wires()
    assert cd.verify(cd.prove(good, _NO_PIS)) == (True, "")
    accepted = []
    for j in range(egc.NUM_CONSTRAINTS[gate]):
        cell, row = egc.constraint_cell(gate, j), j % 2
        bad = good.copy()
        bad[cell, row] = (int(bad[cell, row]) + 1) % P
        ok, _ = cd.verify(cd.prove(bad, _NO_PIS))
        if ok:
            accepted.append(j)
    assert accepted == []


def _check_chained(p, ch, ctx):
    c = ch.circuit
    for name, got, want in ch.results:
        assert got == want, name
    d = c.desc
    assert d.num_gates == 8 and d.num_selectors == 2 and sorted(d.gate_types[:8]) == [0, 1, 2, 3, 10, 11, 12, 13]
    assert (c.constants[:2] == egc.UNUSED_SELECTOR).any()
    cd = _build(p, c, ctx)
    proof = cd.prove(c.wires(), _NO_PIS).to_bytes()
    assert cd.verify(proof) == (True, "")
    return cd, proof


@pytest.mark.gpu
@pytest.mark.parametrize("degree_bits,hasher", [(4, 0), (6, 0), (4, 1)], ids=["n16", "n64_one_fri_round", "n16_keccak"])
def test_all_four_gates_chained_in_one_circuit(gpu, degree_bits, hasher):
    p, ctx = gpu
    ch = egc.Chained(seed=3, min_degree_bits=degree_bits, hasher=hasher)
    assert ch.circuit.n == 1 << degree_bits and ch.circuit.desc.num_fri_rounds == (1 if degree_bits == 6 else 0)
    assert egc.Chained(seed=3, min_degree_bits=5).circuit.desc.num_fri_rounds == 0       # 64 is the smallest n with a FRI reduction
    cd, proof = _check_chained(p, ch, ctx)
    bad = ch.circuit.wires()
    r, col = next((r, 4) for r, row in enumerate(ch.circuit.rows) if row[0] == MUL_EXT)
    bad[col, r] = (int(bad[col, r]) + 1) % P                           # the first MulExtensionGate output, which later rows copy
    assert not cd.verify(cd.prove(bad, _NO_PIS))[0]


@pytest.mark.gpu
def test_phase_api_with_external_transcript_on_the_chained_circuit(gpu, orc):
    # gl_quotient_polys reaches the same launch as gl_prove
    p, ctx = gpu
    c = egc.Chained(seed=4).circuit
    cd = _build(p, c, ctx)
    r = drive_phase_api(p, ctx, orc, cd, poseidon_challenger(orc), c.wires(), _NO_PIS)
    assert r.bytes == cd.prove(c.wires(), _NO_PIS).to_bytes()
    assert cd.verify(r.bytes) == (True, "")


@pytest.mark.gpu
def test_concurrent_proofs_of_the_chained_circuit_on_four_contexts(gpu):
    p, ctx = gpu
    c = egc.Chained(seed=5).circuit
    cd = _build(p, c, ctx)
    wires = c.wires()
    want = cd.prove(wires, _NO_PIS).to_bytes()
    assert cd.verify(want) == (True, "")
    lanes = [p.api.CircuitView(cd, p.Context(device=0)) for _ in range(4)]
    results, errors = {}, []

    def work(lane):
        try:
            results[lane] = lanes[lane].prove(wires, _NO_PIS).to_bytes()
        except Exception as e:          # surfaced below: an assertion inside a thread would be lost
            errors.append(e)

    ths = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    assert not errors, errors
    assert [results[i] == want for i in range(4)] == [True] * 4


# ------------------------------------------------------------------------------- CPU
def _descs():
    out = [(NAMES[g], egc.isolated([g], seed=30 + g).desc, [g]) for g in NEW_GATES]
    out.append(("all_four", _fixture_circuit().desc, NEW_GATES))
    out.append(("chained_two_selector_groups", egc.Chained(seed=6).circuit.desc, NEW_GATES))
    return out


@pytest.mark.parametrize("name,desc,gates", _descs(), ids=[x[0] for x in _descs()])
def test_common_data_bytes_round_trip_and_gate_entries(name, desc, gates):
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    by = api.common_data_to_bytes(desc)
    back, used = api.common_data_from_bytes(by)
    assert used == len(by) and bytes(back) == bytes(desc)
    assert api.common_data_to_bytes(back) == by
    for g in gates:
        tag, param = egc.SERIAL_TAG[g]
        entry = tag.to_bytes(4, "little") + param.to_bytes(8, "little")
        at = by.find(entry)
        assert at > 0 and by.find(entry, at + 1) == -1, NAMES[g]
        for other in (param - 1, param + 1):                          # 9 ops, 44 coefficients, ...
            bad = by[:at + 4] + other.to_bytes(8, "little") + by[at + 12:]
            with pytest.raises(p.Plonky2Mi355xError) as e:
                api.common_data_from_bytes(bad)
            assert e.value.code == 3, NAMES[g]


def test_a_gate_list_out_of_the_builders_order_is_refused():
    # common_data.gates is sorted by (degree, id) (circuit_builder.rs:987): the byte form represents nothing else.  ReducingGate (degree
    # 2) swapped with ArithmeticExtensionGate (degree 3), and ReducingExtensionGate with ReducingGate (equal degree, id order)
    import copy
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    good = _fixture_circuit().desc
    types = list(good.gate_types[:good.num_gates])
    assert types == [0, 1, 2, REDUCING_EXT, REDUCING, ARITHMETIC_EXT, MUL_EXT]
    by = api.common_data_to_bytes(good)
    for i, j in ((4, 5), (3, 4)):
        d = copy.copy(good)
        d.gate_types[i], d.gate_types[j] = types[j], types[i]
        with pytest.raises(p.Plonky2Mi355xError) as e:
            api.common_data_to_bytes(d)
        assert e.value.code == 3
        ea, eb = (b"".join(t.to_bytes(4, "little") + n.to_bytes(8, "little") for t, n in [egc.SERIAL_TAG[types[k]]]) for k in (i, j))
        at = by.find(ea + eb)
        assert at > 0
        with pytest.raises(p.Plonky2Mi355xError) as e:
            api.common_data_from_bytes(by[:at] + eb + ea + by[at + 24:])
        assert e.value.code == 3


def test_gate_type_constants_are_exported():
    # all fourteen codes of the C enum (csrc/gates.hpp, the one place that defines them) against the names _lib.py spells out
    import re
    from plonky2_demo_amd import _lib, api
    assert (api.G_ARITHMETIC_EXT, api.G_MUL_EXT, api.G_REDUCING, api.G_REDUCING_EXT) == (10, 11, 12, 13)
    assert (ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT) == (10, 11, 12, 13)
    with open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc", "gates.hpp")) as f:
        enum = re.search(r"enum \{ (G_NOOP = 0,.*?G_LAST = (\w+)) \};", f.read(), re.S)
    codes = {name: int(value) for name, value in re.findall(r"(G_\w+) = (\d+)", enum.group(1))}
    assert len(codes) == 14 and sorted(codes.values()) == list(range(14)) and codes[enum.group(2)] == 13
    assert {name: getattr(_lib, name) for name in codes} == codes
    assert sorted(n for n in vars(_lib) if re.fullmatch(r"G_[A-Z_]+", n)) == sorted(codes)


# ---- the gate table (csrc/gates.hpp) against counts written from the reference, one gate type at a time ----
NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC, POSEIDON, BASE_SUM, LOOKUP, LOOKUP_TABLE, EXPONENTIATION, RANDOM_ACCESS = range(10)


def _random_access_constraints(bits):
    # RandomAccessGate::new_from_config and num_constraints (gates/random_access.rs:55-72, 285-288) under standard_recursion_config
    vec = 1 << bits
    copies = min(80 // (2 + vec), 135 // (2 + vec + bits))
    return copies * (bits + 2) + min(80 - (2 + vec) * copies, 2)


# num_constraints() of every gate in its new_from_config layout: constant.rs:88-90 (num_consts = 2), public_input.rs:89-91,
# arithmetic_base.rs:119-121 (num_ops = 80 / 4), poseidon.rs:403-409 (12 x 7 full-round and 22 partial-round S-box inputs, 12 outputs, the
# swap bit and its 4 deltas), base_sum.rs:144-146 (1 + 63 limbs), lookup.rs:72-75 and lookup_table.rs (none on the main trace),
# exponentiation.rs:190-192 (66 + 1); the four extension gates from the model's own table.  The oracle has no call that returns a gate's
# count (its gates answer num_constraints() only inside its own circuits), so the numbers are written out here from the reference's
# source, a statement independent of the C++ table.  For the Constant and Arithmetic gates the serialiser takes the count from the
# description, not from the row: the row's figure for those two is held by gl_verify's count check alone
_NUM_CONSTRAINTS = {NOOP: 0, CONSTANT: 2, PUBLIC_INPUT: 4, ARITHMETIC: 80 // 4, POSEIDON: 12 * 7 + 22 + 12 + 1 + 4, BASE_SUM: 1 + 63, LOOKUP: 0,
                    LOOKUP_TABLE: 0, EXPONENTIATION: 66 + 1, **egc.NUM_CONSTRAINTS}
_TABLE_CASES = [(g, 0) for g in range(14) if g != RANDOM_ACCESS] + [(RANDOM_ACCESS, bits) for bits in range(1, 7)]


def _one_gate_desc(gate, param):
    """NoopGate and `gate` alone, one selector group, n = 8; a lookup gate brings its table and the table's other gate (the byte form
    has no table without both).  In build()'s order: degree, then id ("LookupGate" < "LookupTableGate" < "NoopGate")."""
    import copy
    d = copy.copy(egc.isolated([ARITHMETIC_EXT], seed=1, rows_per_gate=1).desc)
    lookups = gate in (LOOKUP, LOOKUP_TABLE)
    gates = [LOOKUP, LOOKUP_TABLE, NOOP] if lookups else [NOOP] if gate == NOOP else [NOOP, gate]
    d.num_gates, d.num_selectors = len(gates), 1
    for i in range(16):
        live = i < len(gates)
        d.gate_types[i], d.gate_params[i] = (gates[i], param if gates[i] == gate else 0) if live else (0, 0)
        d.gate_selector_index[i], d.gate_group_start[i], d.gate_group_end[i] = 0, 0, len(gates) if live else 0
    if lookups:
        d.num_luts, d.num_lookup_polys, d.num_lookup_selectors, d.lut_len[0] = 1, 7, 5, 3
        for j, v in enumerate((0, 5, 1, 6, 2, 7)):
            d.lut[j] = v
        d.last_lut_row[0] = d.first_lut_row[0] = 4          # three entries fill one LookupTableGate row
    d.num_constants = d.num_selectors + d.num_lookup_selectors + 2
    return d


@pytest.mark.parametrize("gate,param", _TABLE_CASES, ids=["type%d_param%d" % c for c in _TABLE_CASES])
def test_gate_table_round_trips_and_counts_constraints_like_the_reference(gate, param):
    from plonky2_demo_amd import api
    d = _one_gate_desc(gate, param)
    by = api.common_data_to_bytes(d)
    back, used = api.common_data_from_bytes(by)
    assert used == len(by) and api.common_data_to_bytes(back) == by
    types = list(back.gate_types[:back.num_gates])
    assert types == list(d.gate_types[:d.num_gates]) and gate in types and back.gate_params[types.index(gate)] == param
    # num_gate_constraints: behind it come num_constants, num_public_inputs, the 80 k_is with their length, num_partial_products, the three
    # lookup counts and the tables (a length and four bytes per entry each)
    tail = 8 * (2 + 81 + 1 + 3) + sum(8 + 4 * d.lut_len[t] for t in range(d.num_luts))
    want = _random_access_constraints(param) if gate == RANDOM_ACCESS else _NUM_CONSTRAINTS[gate]
    assert int.from_bytes(by[-tail - 8:-tail], "little") == want
    assert int.from_bytes(by[-tail - 16:-tail - 8], "little") == d.quotient_degree_factor      # (the word before it: the offset is right)


def _fixture():
    with open(os.path.join(GOLDEN, "ext_gates_n8_proof.bin"), "rb") as f:
        proof = f.read()
    with open(os.path.join(GOLDEN, "ext_gates_n8_verifier_only.bin"), "rb") as f:
        vo = f.read()
    return proof, vo


def test_cpu_verifier_accepts_the_stored_gpu_proof_and_rejects_flipped_openings():
    # a GPU-made proof of the n = 8 circuit with one row of each of the four gates (tests/golden/ext_gates_n8_proof.bin, 69 952 bytes,
    # written by tools/make_ext_gates_fixture.py, with the
    # VerifierOnlyCircuitData bytes = constants_sigmas_cap + circuit digest beside it); the description is rebuilt by the helper
    import plonky2_demo_amd as p
    from plonky2_demo_amd import api
    proof, vo = _fixture()
    c = _fixture_circuit()
    d = c.desc
    assert c.n == 8 and d.num_selectors == 1 and sorted(d.gate_types[:d.num_gates]) == [0, 1, 2, 10, 11, 12, 13]
    cap, digest, used = api.verifier_only_from_bytes(vo)
    assert used == len(vo)
    buf = np.frombuffer(proof, dtype=np.uint8)

    def verify(by):
        b = np.frombuffer(bytes(by), dtype=np.uint8)
        return api._verdict(api.lib.gl_verify(api.ctypes.byref(d), api._p(cap), api._p(digest), api._p(b), b.size))

    assert verify(buf) == (True, "")
    assert api.verify_bytes(vo + api.common_data_to_bytes(d), proof) == (True, "")
    # openings: behind the three caps of 16 digests; constants, sigmas, wires, Z, Z(g x), partial products, quotient chunks, 2 words each
    start, words = 3 * 16 * 4 * 8, 2 * (d.num_constants + 80 + 135 + 2 + 2 + 18 + 16)
    rs = np.random.RandomState(2024)
    for _ in range(64):
        at, bit = start + int(rs.randint(0, 8 * words)), 1 << int(rs.randint(0, 8))
        bad = bytearray(proof)
        bad[at] ^= bit
        assert not verify(bad)[0], (at, bit)
