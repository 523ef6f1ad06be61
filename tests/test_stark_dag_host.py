"""CPU tests of the host code behind STARK constraints as an expression DAG (csrc/stark_dag.hip and the dispatch in stark.hip):
gl_stark_dag_stats against the model's schedule on every AIR of tests/stark_dag_airs.py, every refusal of gl_stark_dag_check beside the
neighbour it accepts, and gl_stark_dag_verify next to the model verifier on the committed proof tests/golden/stark_dag_sbox2_n32.bin
(tools/make_stark_dag_fixture.py wrote it on the GPU; the GPU test test_the_committed_fixture_is_current holds it current)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fri_openings_model as fom
import stark_dag_airs as da
import stark_dag_model as dm
import stark_model as sm
from stark_airs import ALL, FIRST_ROW, LAST_ROW, TRANSITION
from transcript import poseidon_challenger

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARG, UNSUPPORTED = 1, 3
LOCAL, NEXT, PUBLIC, NODE, CONST = range(5)
ADD, SUB, MUL = range(3)
L0, N0, PUB0, K0 = (LOCAL, 0), (NEXT, 0), (PUBLIC, 0), (CONST, 0)


@pytest.fixture(scope="module")
def p():
    import plonky2_demo_amd
    return plonky2_demo_amd


def config_of(p, air, nc=2):
    c = p.StarkConfig.standard_fast_config()
    c.num_challenges, c.rate_bits = nc, air.rate_bits
    return c


# ------------------------------------------------------------------------------- gl_stark_dag_stats, gl_stark_dag_check on the AIRs
@pytest.mark.parametrize("name", list(da.EVERY))
def test_the_stats_equal_the_models_and_the_check_accepts(p, name):
    dag = da.EVERY[name]
    program, max_live = dm.schedule(dag)
    desc = dm.desc_of(p, dag)
    assert desc.stats() == (max_live, max(dm.degrees(dag)[1]), len(program))
    for nc in (1, 2, 3, 4):
        for degree_bits in (5, 12):
            desc.check(config_of(p, dag, nc), degree_bits)


def test_the_stats_take_null_outs_and_the_entries_null_arguments(p):
    lib = p.api.lib
    desc = dm.desc_of(p, da.alias)
    st, dag = desc.struct(2), desc.dag_struct()
    assert lib.gl_stark_dag_stats(ctypes.byref(st), ctypes.byref(dag), None, None, None) == 0
    params = config_of(p, da.alias).fri_params(5)
    assert lib.gl_stark_dag_stats(None, ctypes.byref(dag), None, None, None) == ARG and lib.gl_stark_dag_stats(ctypes.byref(st), None, None, None, None) == ARG
    assert lib.gl_stark_dag_check(ctypes.byref(st), None, ctypes.byref(params)) == ARG and "null dag" in lib.gl_last_error().decode()
    assert lib.gl_stark_dag_check(None, ctypes.byref(dag), ctypes.byref(params)) == ARG and lib.gl_stark_dag_check(ctypes.byref(st), ctypes.byref(dag), None) == ARG
    code = ctypes.c_uint32(99)
    assert lib.gl_stark_dag_verify(ctypes.byref(st), None, ctypes.byref(params), None, 0, ctypes.byref(code)) == ARG
    assert lib.gl_stark_set_dag_check(None, None) == ARG


# ------------------------------------------------------------------------------- every refusal beside its neighbour
def power(k, kind=LOCAL):
    """nodes whose last has degree k (k >= 2): x, x x, ..."""
    return [(MUL, (kind, 0), (kind, 0))] + [(MUL, (NODE, i), (kind, 0)) for i in range(k - 2)]


def status(p, nodes=None, constraints=None, constants=(5,), degree=3, columns=2, pis=1, challenges=2, pairs=(), rate_bits=1, degree_bits=5, hiding=False,
           arity=None, null=None, both=None):
    """gl_stark_dag_check of one description -> (status, message); the defaults are an accepted degree-3 DAG (q = 2)"""
    nodes = power(3) + [(SUB, N0, (NODE, 1))] if nodes is None else nodes
    constraints = [(TRANSITION, (NODE, len(nodes) - 1))] if constraints is None else constraints
    desc = p.StarkDagDesc(columns, pis, degree, [(op, dm.word(a), dm.word(b)) for op, a, b in nodes], constants, [(f, dm.word(o)) for f, o in constraints], pairs)
    st, dag = desc.struct(challenges), desc.dag_struct()
    if both == "term list":
        st = p.StarkDesc(columns, pis, degree, [(ALL, [(1, [(LOCAL, 0)])])], pairs).struct(challenges)
    elif both:                                                           # num_constraints = 0, but one term table is there
        keep = (ctypes.c_uint32 * 1)(0)
        setattr(st, both, ctypes.cast(keep, ctypes.POINTER(ctypes.c_uint32)))
    if null:
        setattr(dag, null, None)
    config = p.StarkConfig.standard_fast_config()
    config.rate_bits = rate_bits
    params = config.fri_params(degree_bits)
    if arity is not None:
        params = p.FriParams(degree_bits, rate_bits, 4, 16, 84, arity, hiding)
    elif hiding:
        params.hiding = 1
    rc = p.api.lib.gl_stark_dag_check(ctypes.byref(st), ctypes.byref(dag), ctypes.byref(params))
    return rc, (p.api.lib.gl_last_error() or b"").decode() if rc else ""


def one(nodes, filt=ALL):
    return dict(nodes=nodes, constraints=[(filt, (NODE, len(nodes) - 1))])


CHAIN = [(ADD, L0, L0)] + [(ADD, (NODE, i), L0) for i in range(65536)]          # 65537 nodes, one live, degree 1
CASES = [
    # (what, refused keywords, status, message fragment, accepted keywords)
    ("a self reference", one([(ADD, L0, L0), (ADD, (NODE, 1), L0)]), ARG, "no earlier node", one([(ADD, L0, L0), (ADD, (NODE, 0), L0)])),
    ("a forward reference", dict(nodes=[(ADD, L0, (NODE, 1)), (ADD, L0, L0)], constraints=[(ALL, (NODE, 0))]), ARG, "no earlier node",
     dict(nodes=[(ADD, L0, L0), (ADD, L0, (NODE, 0))], constraints=[(ALL, (NODE, 0))])),
    ("a self reference in b", one([(MUL, L0, (NODE, 0))]), ARG, "no earlier node", one([(MUL, L0, L0)])),
    ("an unknown op", one([(3, L0, L0)]), ARG, "unknown op", one([(MUL, L0, L0)])),
    ("an unknown operand kind", one([(ADD, (5, 0), L0)]), ARG, "operand kind", one([(ADD, K0, L0)])),
    ("an unknown kind in a constraint", dict(nodes=[], constraints=[(ALL, (15, 0))]), ARG, "operand kind", dict(nodes=[], constraints=[(ALL, K0)])),
    ("a column index out of range", one([(ADD, (LOCAL, 2), L0)]), ARG, "column index", one([(ADD, (LOCAL, 1), L0)])),
    ("a next-row column out of range", one([(ADD, L0, (NEXT, 2))]), ARG, "column index", one([(ADD, L0, (NEXT, 1))])),
    ("a public-input index out of range", one([(ADD, (PUBLIC, 1), L0)]), ARG, "public-input index", one([(ADD, PUB0, L0)])),
    ("a public input where there are none", dict(pis=0, **one([(ADD, PUB0, L0)])), ARG, "public-input index", dict(pis=0, **one([(ADD, L0, L0)]))),
    ("a constant index out of range", one([(ADD, (CONST, 1), L0)]), ARG, "constant index", one([(ADD, K0, L0)])),
    ("a constant where there are none", dict(constants=(), **one([(ADD, K0, L0)])), ARG, "constant index", dict(constants=(), **one([(ADD, L0, L0)]))),
    ("a constraint on a node that is not there", dict(nodes=[(ADD, L0, L0)], constraints=[(ALL, (NODE, 1))]), ARG, "node index", dict(nodes=[(ADD, L0, L0)], constraints=[(ALL, (NODE, 0))])),
    ("a node index out of range in a node", one([(ADD, L0, (NODE, 7))]), ARG, "node index", one([(ADD, L0, L0)])),
    ("an unknown filter", dict(nodes=[], constraints=[(4, L0)]), ARG, "filter", dict(nodes=[], constraints=[(LAST_ROW, L0)])),
    ("no constraints", dict(nodes=[], constraints=[]), ARG, "constraints", dict(nodes=[], constraints=[(ALL, L0)])),
    ("too many constraints", dict(nodes=[], constraints=[(ALL, L0)] * 4097), ARG, "constraints", dict(nodes=[], constraints=[(ALL, L0)] * 4096)),
    ("too many nodes", one(CHAIN), ARG, "65536 nodes", one(CHAIN[:65536])),
    ("too many constants", dict(constants=[1] * 65537), ARG, "65536 constants", dict(constants=[1] * 65536)),
    # the degree rule at q = 2: q + 1 under ALL / TRANSITION, q under a row filter; PUBLIC and CONST count nothing, ADD takes the maximum
    ("degree q + 2 on all rows", one(power(4)), ARG, "degree is above", one(power(3))),
    ("degree q + 2 on transitions", one(power(4, NEXT), TRANSITION), ARG, "degree is above", one(power(3, NEXT), TRANSITION)),
    ("degree q + 1 on the first row", one(power(3), FIRST_ROW), ARG, "degree is above", one(power(2), FIRST_ROW)),
    ("degree q + 1 on the last row", one(power(3), LAST_ROW), ARG, "degree is above", one(power(2), LAST_ROW)),
    ("a product of two squares", one(power(2) + [(MUL, (NODE, 0), (NODE, 0))]), ARG, "degree is above", one(power(2) + [(ADD, (NODE, 0), (NODE, 0))])),
    ("q + 2 beside public and constant factors", one(power(4) + [(MUL, (NODE, 2), PUB0), (MUL, (NODE, 3), K0)]), ARG, "degree is above",
     one(power(3) + [(MUL, (NODE, 1), PUB0), (MUL, (NODE, 2), K0), (MUL, (NODE, 3), PUB0)])),
    ("a bare column on the first row at q = 1 is on the bound", dict(degree=2, **one(power(2), FIRST_ROW)), ARG, "degree is above",
     dict(degree=2, nodes=[], constraints=[(FIRST_ROW, L0)])),
    # one form or the other
    ("a term list beside the dag", dict(both="term list"), ARG, "term list as well", dict()),
] + [("a term table (%s) beside the dag" % f, dict(both=f), ARG, "term list as well", dict())
     for f in ("constraint_filter", "constraint_num_terms", "term_num_factors", "factors")] + [
    ("a null %s" % f, dict(null=f), ARG, "null", dict()) for f in ("node_op", "node_a", "node_b", "constants", "constraint_filter", "constraint_operand")] + [
    # what gl_stark_check refuses in the rest of the description and in the params, reached through the new entry
    ("no columns", dict(columns=0), ARG, "columns", dict(columns=1, nodes=[], constraints=[(ALL, L0)])),
    ("too many columns", dict(columns=1025), ARG, "columns", dict(columns=1024)),
    ("too many public inputs", dict(pis=257), ARG, "public inputs", dict(pis=256)),
    ("degree 0", dict(degree=0), ARG, "constraint degree", dict(degree=1, nodes=[], constraints=[(ALL, L0)])),
    ("degree 10", dict(degree=10, rate_bits=3), ARG, "constraint degree", dict(degree=9, rate_bits=3)),
    ("no challenges", dict(challenges=0), ARG, "challenges", dict(challenges=1)),
    ("five challenges", dict(challenges=5), ARG, "challenges", dict(challenges=4)),
    ("too many pairs", dict(pairs=[[(0, 1)]] * 65), ARG, "permutation pairs", dict(pairs=[[(0, 1)]] * 64)),
    ("an empty pair", dict(pairs=[[]]), ARG, "column pairs", dict(pairs=[[(0, 1)]])),
    ("a permutation column out of range", dict(pairs=[[(0, 2)]]), ARG, "permutation column", dict(pairs=[[(0, 1)]])),
    ("hiding", dict(hiding=True), UNSUPPORTED, "hiding", dict(hiding=False)),
    ("a degree above the rate", dict(degree=4), UNSUPPORTED, "higher than the rate", dict(degree=4, rate_bits=2)),
    ("an arity other than 16", dict(arity=[3], degree_bits=7), UNSUPPORTED, "arity must be 16", dict(arity=[4], degree_bits=7)),
]


@pytest.mark.parametrize("what,refused,code,fragment,accepted", CASES, ids=[c[0] for c in CASES])
def test_gl_stark_dag_check_refuses_and_accepts_the_neighbour(p, what, refused, code, fragment, accepted):
    rc, message = status(p, **refused)
    assert rc == code and fragment in message, "%s: status %d, %r" % (what, rc, message)
    assert status(p, **accepted) == (0, ""), "%s: the neighbour beside it is refused" % what


def test_the_live_cap_on_the_bound_and_one_beyond(p):
    config = config_of(p, da.at_cap())
    dm.desc_of(p, da.at_cap()).check(config, 5)
    assert dm.desc_of(p, da.at_cap()).stats()[0] == p.GL_STARK_DAG_MAX_LIVE == 128
    for entry in (lambda d: d.check(config, 5), lambda d: d.stats()):
        with pytest.raises(p.Plonky2Mi355xError, match="128 values live") as e:
            entry(dm.desc_of(p, da.at_cap(129)))
        assert e.value.code == ARG


def test_gl_stark_check_without_a_dag_still_refuses_zero_constraints(p):
    desc = dm.desc_of(p, da.alias)
    params = config_of(p, da.alias).fri_params(5)
    assert p.api.lib.gl_stark_check(ctypes.byref(desc.struct(2)), ctypes.byref(params)) == ARG
    assert "1..4096 constraints" in p.api.lib.gl_last_error().decode()
    empty = p.StarkDesc(4, 0, 3, [], []).struct(2)                       # no constraints, the term tables there
    assert p.api.lib.gl_stark_check(ctypes.byref(empty), ctypes.byref(params)) == ARG
    code = ctypes.c_uint32()
    assert p.api.lib.gl_stark_verify(ctypes.byref(desc.struct(2)), ctypes.byref(params), None, 0, ctypes.byref(code)) == ARG
    assert p.api.lib.gl_stark_dag_check(ctypes.byref(desc.struct(2)), ctypes.byref(desc.dag_struct()), ctypes.byref(params)) == 0


def test_a_set_takes_a_dag_per_table_and_refuses_what_the_single_entry_refuses(p):
    import stark_ctl_airs as ca
    lib = p.api.lib
    lgs, config = [5, 6, 5], ca.config(p, 2)
    plain, mixed = da.api_set(p, lgs, config, dag_tables=()), da.api_set(p, lgs, config)
    assert [isinstance(d, p.StarkDagDesc) for d, _ in mixed.tables] == [False, False, True] and plain.dags()[0] is None
    # the entry with null dags, and with every entry null, is gl_stark_set_check
    plain.check()
    assert lib.gl_stark_set_dag_check(ctypes.byref(plain.struct()), None) == 0
    assert lib.gl_stark_set_dag_check(ctypes.byref(plain.struct()), (ctypes.c_void_p * 3)()) == 0
    mixed.check()
    assert [mixed.num_zs(t) for t in range(3)] == [plain.num_zs(t) for t in range(3)]
    # a table in DAG form without its dag is a table without constraints
    assert lib.gl_stark_set_check(ctypes.byref(mixed.struct())) == ARG and "1..4096 constraints" in lib.gl_last_error().decode()
    # a dag beside a table that carries a term list
    dags, keep = mixed.dags()
    assert lib.gl_stark_set_dag_check(ctypes.byref(plain.struct()), dags) == ARG and "term list as well" in lib.gl_last_error().decode()
    # the DAG's own rules, per table: a constraint above the degree rule in the mul table
    d = mixed.tables[ca.MUL][0]
    mixed.tables[ca.MUL] = (p.StarkDagDesc(d.num_columns, d.num_public_inputs, 2, d.nodes, d.constants, d.dag_constraints, d.pairs), 5)
    with pytest.raises(p.Plonky2Mi355xError, match="degree is above"):
        mixed.check()
    code, table = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.gl_stark_set_dag_verify(None, None, None, 0, ctypes.byref(code), ctypes.byref(table)) == ARG


# ------------------------------------------------------------------------------- the committed proof
STEM = "stark_dag_sbox2_n32"


@pytest.fixture(scope="module")
def fixture(p):
    with open(os.path.join(GOLDEN, STEM + ".bin"), "rb") as f:
        proof = f.read()
    with open(os.path.join(GOLDEN, STEM + ".json")) as f:
        meta = json.load(f)
    air = da.EVERY[meta["air"]]
    config = config_of(p, air, meta["num_challenges"])
    params = config.fri_params(meta["params"]["degree_bits"])
    assert {k: getattr(params, k) for k in meta["params"]} == meta["params"] and meta["num_bytes"] == len(proof)
    assert (air.name, air.q, meta["num_challenges"], params.rate_bits, params.degree_bits) == ("sbox2", 8, 2, 3, 5)
    return proof, meta, dm.desc_of(p, air), config, params, air, meta["num_challenges"]


def library(p, fixture, proof):
    _, meta, desc, config = fixture[:4]
    ok, why, code = p.stark_dag_verify(desc, config, meta["params"]["degree_bits"], proof)
    assert ok == (code == 0) and (ok, why, code) == p.stark_verify(desc, config, meta["params"]["degree_bits"], proof)
    return code


def model(orc, fixture, proof):
    params, air, nc = fixture[4:7]
    return dm.verify(air, nc, params, proof, poseidon_challenger(orc), fom.poseidon_verify_path(orc))


def layout(params, air, nc):
    """(region name, first byte, length, in the transcript?, the check a flip there fails or None): no pairs, so two oracles; 2^5: no reduction"""
    cap = 32 << params.cap_height
    assert not air.pairs and not params.reduction_arity_bits
    siblings = params.degree_bits + params.rate_bits - params.cap_height
    regions, at = [], 0

    def add(name, length, transcript, check):
        nonlocal at
        regions.append((name, at, length, transcript, check))
        at += length
    for name in ("trace_cap", "quotient_polys_cap"):
        add(name, cap, True, None)
    for name, k in (("local_values", air.num_columns), ("next_values", air.num_columns), ("quotient_polys", air.q * nc)):
        add(name, 16 * k, True, None)
    for q in range(params.num_query_rounds):
        for o, k in enumerate((air.num_columns, air.q * nc)):
            add("query %d leaf %d" % (q, o), 8 * k, False, fom.INITIAL_MERKLE)
            add("query %d path length %d" % (q, o), 1, False, "decode")
            add("query %d siblings %d" % (q, o), 32 * siblings, False, fom.INITIAL_MERKLE)
    add("final_poly", 16 << params.degree_bits, True, None)
    add("pow_witness", 8, True, None)
    add("public_inputs", 8 * air.num_public_inputs, False, fom.VANISHING)
    return regions, at


def test_the_fixture_is_accepted_by_the_library_and_by_the_model(p, orc, fixture):
    proof, meta, _, _, params, air, nc = fixture
    regions, size = layout(params, air, nc)
    assert size == len(proof)
    assert library(p, fixture, proof) == 0 and model(orc, fixture, proof) == 0
    pp = sm.ParsedStarkProof(air, nc, params, proof)
    assert pp.public_inputs == meta["public_inputs"] == air.trace(meta["num_rows"], seed=meta["trace_seed"])[1]
    assert (pp.trace_cap[0], pp.quotient_cap[0], pp.zs_cap, len(pp.quotient)) == (meta["trace_cap_first_words"], meta["quotient_polys_cap_first_words"], None, 16)


def test_the_fixture_changed_anywhere_is_rejected_by_both_with_the_same_check(p, orc, fixture):
    proof, _, _, _, params, air, nc = fixture
    regions, _ = layout(params, air, nc)
    rng = np.random.Generator(np.random.PCG64(2026))
    by_kind = {}
    for r in regions:
        by_kind.setdefault(r[0].split(" ", 2)[-1] if r[0].startswith("query") else r[0], []).append(r)
    assert len(by_kind) == 14
    picks = [(rs[int(rng.integers(0, len(rs)))], 0, None) for rs in by_kind.values()]          # every cap, opening family and part of a query
    named = {r[0]: r for r in regions}
    quotient = named["quotient_polys"]
    picks += [(quotient, 16 * k, 16) for k in (0, air.q - 1, air.q, 2 * air.q - 1)]             # the first and the last chunk of each challenge
    picks += [(named["local_values"], 16 * c, 16) for c in (0, air.num_columns - 1)] + [(named["next_values"], 16 * c, 16) for c in (0, air.num_columns - 1)]
    picks += [(named["public_inputs"], 8 * i, 8) for i in (0, air.num_columns - 1, air.num_columns)]      # first-row ones and the last-row one
    for (name, first, length, transcript, check), at, span in picks:
        byte, bit = first + at + int(rng.integers(0, span or length)), int(rng.integers(0, 8))
        if "path length" in name:
            bit = int(rng.integers(0, 3))
        bad = bytearray(proof)
        bad[byte] ^= 1 << bit
        got, want = library(p, fixture, bytes(bad)), model(orc, fixture, bytes(bad))
        assert got != 0 and got == want, "bit %d of byte %d (%s): the library says %d, the model %d" % (bit, byte, name, got, want)
        if not transcript and check != "decode":
            assert got == check, "bit %d of byte %d (%s): check %d, not %d" % (bit, byte, name, got, check)
        if check == "decode":
            assert got in (fom.TRUNCATED, fom.LENGTH, fom.INITIAL_PATH_LENGTH)


def test_the_fixture_truncated_or_with_a_trailing_byte(p, orc, fixture):
    proof = fixture[0]
    for cut in (1, 8, 16, 17, len(proof) - 100, len(proof)):
        assert library(p, fixture, proof[:len(proof) - cut]) == fom.TRUNCATED == model(orc, fixture, proof[:len(proof) - cut])
    assert library(p, fixture, proof + b"\0") == fom.LENGTH == model(orc, fixture, proof + b"\0")


def test_another_dag_does_not_verify_the_fixture(p, fixture):
    # one constant of the second round changed: the same shape, another AIR
    proof, meta, desc, config = fixture[:4]
    other = p.StarkDagDesc(desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.nodes, desc.constants[:-1] + [desc.constants[-1] + 1],
                           desc.dag_constraints, desc.pairs)
    ok, why, code = p.stark_dag_verify(other, config, meta["params"]["degree_bits"], proof)
    assert (ok, code) == (False, fom.VANISHING) and "anishing" in why


# ------------------------------------------------------------------------------- the compiler's report
def test_every_dag_kernel_compiles_without_scratch_and_the_committed_report_is_current():
    # Node values live in LDS slots, never in a runtime-indexed private array, so no instantiation may need scratch.  The compiler is asked
    # here (device code only, a few seconds, no GPU), and profiles/stark_dag_resource_usage.txt must be what it answers: the report is made
    # by `make -s -C plonky2_demo_amd/csrc stark_dag.resource_usage` and compared with the source positions left out.
    root = os.path.dirname(os.path.dirname(GOLDEN))
    report = subprocess.run(["make", "-s", "-C", os.path.join(root, "plonky2_demo_amd", "csrc"), "stark_dag.resource_usage"], capture_output=True, text=True, timeout=300)
    assert report.returncode == 0, report.stderr
    names = re.findall(r"Function Name: (\S+)", report.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report.stdout)]
    static_lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", report.stdout)]
    assert len(names) == len(scratch) == len(static_lds) == 4 and not any(scratch), report.stdout
    assert not any(static_lds)                                            # the slots are dynamic LDS, sized by the launch to the program's max live
    assert all("k_stark_quotient_dag" in n for n in names) and len(set(names)) == 4
    with open(os.path.join(root, "profiles", "stark_dag_resource_usage.txt")) as f:
        committed = f.read()
    unplaced = lambda text: re.sub(r"(?m)^\S+?:\d+:\d+: ", "", text)      # noqa: E731
    assert unplaced(committed) == unplaced(report.stdout), "profiles/stark_dag_resource_usage.txt is stale"
