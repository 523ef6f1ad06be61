"""CPU tests of the STARK seam's host code (csrc/stark.hip): gl_stark_check's refusals, each beside the boundary case it accepts, and
gl_stark_verify on the committed proofs tests/golden/stark_fibonacci_n32.bin (two challenges, q = 1) and stark_nonic_n32_nc3.bin (three
challenges, q = 8 at rate_bits 3) next to the model verifier of tests/stark_model.py.  tools/make_stark_fixture.py wrote them on the GPU;
the GPU tests test_the_committed_*fixture_is_current hold them current."""
import ctypes
import json
import os

import numpy as np
import pytest

import fri_openings_model as fom
import stark_airs
import stark_model as sm
from stark_airs import ALL, FIRST_ROW, LAST_ROW, LOCAL, NEXT, PUBLIC, TRANSITION
from transcript import poseidon_challenger

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARG, UNSUPPORTED = 1, 3
L0, N0, PUB0 = (LOCAL, 0), (NEXT, 0), (PUBLIC, 0)


@pytest.fixture(scope="module")
def p():
    import plonky2_demo_amd
    return plonky2_demo_amd


# ------------------------------------------------------------------------------- gl_stark_check
def status(p, degree=3, columns=2, pis=1, challenges=2, constraints=None, pairs=(), rate_bits=1, degree_bits=5, arity=None, hiding=False,
           null=None, cap_height=4):
    """gl_stark_check of one description -> (status, message); the defaults are an accepted degree-3 AIR (q = 2)"""
    constraints = [(TRANSITION, [(1, [N0]), (5, [L0, L0, L0])])] if constraints is None else constraints
    st = p.StarkDesc(columns, pis, degree, constraints, pairs).struct(challenges)
    if null:
        setattr(st, null, None)
    config = p.StarkConfig.standard_fast_config()
    config.rate_bits = rate_bits
    params = config.fri_params(degree_bits)
    if arity is not None:
        params = p.FriParams(degree_bits, rate_bits, cap_height, 16, 84, arity, hiding)
    elif hiding:
        params.hiding = 1
    rc = p.api.lib.gl_stark_check(ctypes.byref(st), ctypes.byref(params))
    return rc, (p.api.lib.gl_last_error() or b"").decode() if rc else ""


def term(k, kind=LOCAL, extra=()):
    return (1, [(kind, 0)] * k + list(extra))


CASES = [
    # (what, refused keywords, status, message fragment, accepted keywords)
    ("no columns", dict(columns=0), ARG, "columns", dict(columns=1)),
    ("too many columns", dict(columns=1025), ARG, "columns", dict(columns=1024)),
    ("too many public inputs", dict(pis=257), ARG, "public inputs", dict(pis=256)),
    ("degree 0", dict(degree=0), ARG, "constraint degree", dict(degree=1, constraints=[(ALL, [term(2)])])),
    ("degree 10", dict(degree=10, rate_bits=3), ARG, "constraint degree", dict(degree=9, rate_bits=3)),
    ("no challenges", dict(challenges=0), ARG, "challenges", dict(challenges=1)),
    ("five challenges", dict(challenges=5), ARG, "challenges", dict(challenges=4)),
    ("no constraints", dict(constraints=[]), ARG, "constraints", dict(constraints=[(ALL, [])])),
    ("too many constraints", dict(constraints=[(ALL, [])] * 4097), ARG, "constraints", dict(constraints=[(ALL, [])] * 4096)),
    ("too many terms", dict(constraints=[(ALL, [term(1)] * 32769), (ALL, [term(1)] * 32768)]), ARG, "terms", dict(constraints=[(ALL, [term(1)] * 32768)] * 2)),
    ("too many factors in a term", dict(constraints=[(ALL, [term(3, extra=[PUB0] * 62)])]), ARG, "64 factors", dict(constraints=[(ALL, [term(3, extra=[PUB0] * 61)])])),
    ("too many pairs", dict(pairs=[[(0, 1)]] * 65), ARG, "permutation pairs", dict(pairs=[[(0, 1)]] * 64)),
    ("an empty pair", dict(pairs=[[]]), ARG, "column pairs", dict(pairs=[[(0, 1)]])),
    ("a pair of 65 column pairs", dict(pairs=[[(0, 1)] * 65]), ARG, "column pairs", dict(pairs=[[(0, 1)] * 64])),
    ("a permutation column out of range", dict(pairs=[[(0, 2)]]), ARG, "permutation column", dict(pairs=[[(0, 1)]])),
    ("a column index out of range", dict(constraints=[(ALL, [(1, [(LOCAL, 2)])])]), ARG, "column index", dict(constraints=[(ALL, [(1, [(NEXT, 1)])])])),
    ("a public-input index out of range", dict(constraints=[(ALL, [(1, [(PUBLIC, 1)])])]), ARG, "public-input index", dict(constraints=[(ALL, [(1, [PUB0])])])),
    ("a public input where there are none", dict(pis=0, constraints=[(ALL, [(1, [PUB0])])]), ARG, "public-input index", dict(pis=0)),
    ("an unknown filter", dict(constraints=[(4, [term(1)])]), ARG, "filter", dict(constraints=[(LAST_ROW, [term(1)])])),
    ("an unknown operand kind", dict(constraints=[(ALL, [(1, [(3, 0)])])]), ARG, "operand kind", dict(constraints=[(ALL, [(1, [PUB0])])])),
    # the degree rule at q = 2: q + 1 trace factors, q under a row filter; public inputs are constants
    ("q + 2 factors on all rows", dict(constraints=[(ALL, [term(4)])]), ARG, "LOCAL / NEXT factors", dict(constraints=[(ALL, [term(3)])])),
    ("q + 2 factors on transitions", dict(constraints=[(TRANSITION, [term(4, NEXT)])]), ARG, "LOCAL / NEXT factors", dict(constraints=[(TRANSITION, [term(3, NEXT)])])),
    ("q + 1 factors on the first row", dict(constraints=[(FIRST_ROW, [term(3)])]), ARG, "LOCAL / NEXT factors", dict(constraints=[(FIRST_ROW, [term(2)])])),
    ("q + 1 factors on the last row", dict(constraints=[(LAST_ROW, [term(3)])]), ARG, "LOCAL / NEXT factors", dict(constraints=[(LAST_ROW, [term(2)])])),
    ("q + 2 factors beside public ones", dict(constraints=[(ALL, [term(4, extra=[PUB0])])]), ARG, "LOCAL / NEXT factors", dict(constraints=[(ALL, [term(3, extra=[PUB0] * 5)])])),
    ("hiding", dict(hiding=True), UNSUPPORTED, "hiding", dict(hiding=False)),
    ("a degree above the rate", dict(degree=4), UNSUPPORTED, "higher than the rate", dict(degree=4, rate_bits=2)),
    ("degree 6 at rate_bits 2", dict(degree=6, rate_bits=2), UNSUPPORTED, "higher than the rate", dict(degree=5, rate_bits=2)),
    ("an arity other than 16", dict(arity=[3], degree_bits=7), UNSUPPORTED, "arity must be 16", dict(arity=[4], degree_bits=7)),
    ("degree_bits 0", dict(arity=[], degree_bits=0, cap_height=0), ARG, "degree_bits", dict(arity=[], degree_bits=1, cap_height=0)),
    ("a reduction above degree_bits", dict(arity=[4, 4], degree_bits=7, cap_height=0), ARG, "reduction arity", dict(arity=[4, 4], degree_bits=8, cap_height=0)),
] + [("a null %s" % field, dict(null=field, pairs=[[(0, 1)]]), ARG, "null", dict(pairs=[[(0, 1)]]))
     for field in ("constraint_filter", "constraint_num_terms", "term_coeff", "term_num_factors", "factors", "pair_len", "pair_columns")]


@pytest.mark.parametrize("what,refused,code,fragment,accepted", CASES, ids=[c[0] for c in CASES])
def test_gl_stark_check_refuses_and_accepts_the_boundary(p, what, refused, code, fragment, accepted):
    rc, message = status(p, **refused)
    assert rc == code and fragment in message, "%s: status %d, %r" % (what, rc, message)
    assert status(p, **accepted) == (0, ""), "%s: the boundary case beside it is refused" % what


def test_gl_stark_check_takes_null_arguments_and_the_four_airs(p):
    # (every AIR of stark_airs.py by now, under each num_challenges)
    assert p.api.lib.gl_stark_check(None, None) == ARG
    for air in stark_airs.AIRS.values():
        config = p.StarkConfig.standard_fast_config()
        config.rate_bits = air.rate_bits
        for nc in (1, 2, 3, 4):
            config.num_challenges = nc
            for degree_bits in (5, 7, 12):
                p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs).check(config, degree_bits)
    # the description api.fibonacci_stark gives is the one the tests' model runs on
    desc, generate = p.fibonacci_stark(32)
    air = stark_airs.fibonacci
    assert (desc.num_columns, desc.num_public_inputs, desc.constraint_degree, desc.constraints, desc.pairs) == \
        (air.num_columns, air.num_public_inputs, air.constraint_degree, [(f, [(c, list(ops)) for c, ops in terms]) for f, terms in air.constraints], air.pairs)
    trace, pis = air.trace(32)
    assert (generate(0, 1) == trace).all() and pis == [0, 1, 2178309]


# ------------------------------------------------------------------------------- the committed proof
NC = 2


def load(p, stem, desc_of):
    """(proof, meta, desc, config, params, air, num_challenges) of a committed proof"""
    with open(os.path.join(GOLDEN, stem + ".bin"), "rb") as f:
        proof = f.read()
    with open(os.path.join(GOLDEN, stem + ".json")) as f:
        meta = json.load(f)
    air = stark_airs.AIRS[meta["air"]]
    config = p.StarkConfig.standard_fast_config()
    config.num_challenges, config.rate_bits = meta["num_challenges"], meta["params"]["rate_bits"]
    params = config.fri_params(meta["params"]["degree_bits"])
    assert {k: getattr(params, k) for k in meta["params"]} == meta["params"] and meta["num_bytes"] == len(proof)
    return proof, meta, desc_of(meta, air), config, params, air, meta["num_challenges"]


@pytest.fixture(scope="module")
def fixture(p):
    f = load(p, "stark_fibonacci_n32", lambda meta, air: p.fibonacci_stark(meta["num_rows"])[0])
    assert f[6] == NC and f[4].rate_bits == 1                            # standard_fast_config as it stands
    return f


@pytest.fixture(scope="module")
def nonic_fixture(p):
    f = load(p, "stark_nonic_n32_nc3", lambda meta, air: p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs))
    assert (f[5].name, f[5].q, f[6], f[4].rate_bits, f[4].degree_bits) == ("nonic", 8, 3, 3, 5)
    return f


def library(p, fixture, proof):
    _, meta, desc, config = fixture[:4]
    ok, why, code = p.stark_verify(desc, config, meta["params"]["degree_bits"], proof)
    assert ok == (code == 0)
    return code


def model(orc, fixture, proof):
    params, air, nc = fixture[4:7]
    return sm.verify(air, nc, params, proof, poseidon_challenger(orc), fom.poseidon_verify_path(orc))


def layout(params, air=stark_airs.fibonacci, nc=NC):
    """(region name, first byte, length, in the transcript?, the check a flip there fails or None) of a proof at 2^5: no FRI reduction"""
    cap, nz = 32 << params.cap_height, sm.num_zs(air, nc)
    assert nz and not params.reduction_arity_bits
    siblings = params.degree_bits + params.rate_bits - params.cap_height
    regions, at = [], 0

    def add(name, length, transcript, check):
        nonlocal at
        regions.append((name, at, length, transcript, check))
        at += length
    for name in ("trace_cap", "permutation_zs_cap", "quotient_polys_cap"):
        add(name, cap, True, None)
    for name, k in (("local_values", air.num_columns), ("next_values", air.num_columns), ("permutation_zs", nz), ("permutation_zs_next", nz),
                    ("quotient_polys", air.q * nc)):
        add(name, 16 * k, True, None)
    for q in range(params.num_query_rounds):
        for o, k in enumerate((air.num_columns, nz, air.q * nc)):
            add("query %d leaf %d" % (q, o), 8 * k, False, fom.INITIAL_MERKLE)
            add("query %d path length %d" % (q, o), 1, False, "decode")
            add("query %d siblings %d" % (q, o), 32 * siblings, False, fom.INITIAL_MERKLE)
    add("final_poly", 16 << params.degree_bits, True, None)
    add("pow_witness", 8, True, None)
    add("public_inputs", 8 * air.num_public_inputs, False, fom.VANISHING)      # this version of the reference does not observe them
    return regions, at


def test_the_fixture_is_accepted_by_the_library_and_by_the_model(p, orc, fixture):
    proof, meta, params = fixture[0], fixture[1], fixture[4]
    regions, size = layout(params)
    assert size == len(proof) == 24060
    assert library(p, fixture, proof) == 0 and model(orc, fixture, proof) == 0
    pp = sm.ParsedStarkProof(stark_airs.fibonacci, NC, params, proof)
    assert pp.public_inputs == meta["public_inputs"]
    assert (pp.trace_cap[0], pp.zs_cap[0], pp.quotient_cap[0]) == (meta["trace_cap_first_words"], meta["permutation_zs_cap_first_words"], meta["quotient_polys_cap_first_words"])


def kinds_of(regions):
    by_kind = {}
    for r in regions:
        by_kind.setdefault(r[0].split(" ", 2)[-1] if r[0].startswith("query") else r[0], []).append(r)
    return by_kind


def test_single_bit_flips_in_every_region_are_rejected_by_both(p, orc, fixture):
    proof, params = fixture[0], fixture[4]
    regions, _ = layout(params)
    rng = np.random.Generator(np.random.PCG64(2024))
    by_kind = kinds_of(regions)
    picks = []
    for kind, rs in by_kind.items():                                     # three flips in every kind of region, 20 kinds ...
        for _ in range(3):
            picks.append(rs[int(rng.integers(0, len(rs)))])
    while len(picks) < 64:                                               # ... and the rest anywhere
        picks.append(regions[int(rng.integers(0, len(regions)))])
    assert len(picks) == 64 and len(by_kind) == 20
    flips_are_rejected_by_both(p, orc, fixture, rng, picks)


def flips_are_rejected_by_both(p, orc, fixture, rng, picks):
    """picks: regions, or (region, first byte inside it, length) to flip within a part of one"""
    proof = fixture[0]
    for pick in picks:
        (name, first, length, transcript, check), at, span = pick if len(pick) == 3 else (pick, 0, pick[2])
        byte, bit = first + at + int(rng.integers(0, span)), int(rng.integers(0, 8))
        if "path length" in name:
            bit = int(rng.integers(0, 3))                                # a length the proof could hold: 2 -> 3, 0 or 6
        bad = bytearray(proof)
        bad[byte] ^= 1 << bit
        got, want = library(p, fixture, bytes(bad)), model(orc, fixture, bytes(bad))
        assert got != 0 and want != 0, "a flipped bit in %s (byte %d) is accepted" % (name, byte)
        assert got == want, "bit %d of byte %d (%s): the library says %d, the model %d" % (bit, byte, name, got, want)
        if not transcript and check != "decode":
            assert got == check, "bit %d of byte %d (%s): check %d, not %d" % (bit, byte, name, got, check)
        if check == "decode":
            assert got in (fom.TRUNCATED, fom.LENGTH, fom.INITIAL_PATH_LENGTH)


def test_truncation_and_a_trailing_byte(p, orc, fixture):
    proof = fixture[0]
    for cut in (1, 8, 24, 25, len(proof) - 100, len(proof)):
        assert library(p, fixture, proof[:len(proof) - cut]) == fom.TRUNCATED == model(orc, fixture, proof[:len(proof) - cut])
    assert library(p, fixture, proof + b"\0") == fom.LENGTH == model(orc, fixture, proof + b"\0")


# ------------------------------------------------------------------------------- the same on three challenges and eight chunks
def test_the_nonic_fixture_is_accepted_by_the_library_and_by_the_model(p, orc, nonic_fixture):
    proof, meta, _, _, params, air, nc = nonic_fixture
    regions, size = layout(params, air, nc)
    assert size == len(proof)
    assert library(p, nonic_fixture, proof) == 0 and model(orc, nonic_fixture, proof) == 0
    pp = sm.ParsedStarkProof(air, nc, params, proof)
    assert pp.public_inputs == meta["public_inputs"] == air.trace(meta["num_rows"], seed=meta["trace_seed"])[1]
    assert (len(pp.zs), len(pp.quotient)) == (2, 24)                     # ceil(3 pairs x 3 challenges / 8), 3 x 8 chunks
    assert (pp.trace_cap[0], pp.zs_cap[0], pp.quotient_cap[0]) == (meta["trace_cap_first_words"], meta["permutation_zs_cap_first_words"], meta["quotient_polys_cap_first_words"])


def test_the_nonic_fixture_changed_anywhere_is_rejected_by_both_with_the_same_check(p, orc, nonic_fixture):
    proof, _, _, _, params, air, nc = nonic_fixture
    regions, _ = layout(params, air, nc)
    rng = np.random.Generator(np.random.PCG64(2025))
    by_kind = kinds_of(regions)
    assert len(by_kind) == 20
    picks = [rs[int(rng.integers(0, len(rs)))] for rs in by_kind.values()]                    # every cap, opening family and part of a query
    named = {r[0]: r for r in regions}
    quotient = named["quotient_polys"]
    assert quotient[2] == 16 * nc * air.q
    picks += [(quotient, 16 * (2 * air.q + k), 16) for k in (0, air.q - 1)]                   # the first and the last chunk of challenge 2 ...
    picks += [(quotient, 16 * (air.q - 1), 16), (named["permutation_zs"], 16, 16), (named["permutation_zs_next"], 16, 16)]      # ... chunk 7, the partial batch's Z
    picks += [(named["public_inputs"], 8 * i, 8) for i in range(air.num_public_inputs)]
    picks += [(named["local_values"], 16 * c, 16) for c in (0, air.num_columns - 1)] + [(named["next_values"], 0, 16)]
    flips_are_rejected_by_both(p, orc, nonic_fixture, rng, picks)


def test_the_nonic_fixture_truncated_or_with_a_trailing_byte(p, orc, nonic_fixture):
    proof = nonic_fixture[0]
    for cut in (1, 8, 16, 17, len(proof) - 100, len(proof)):
        assert library(p, nonic_fixture, proof[:len(proof) - cut]) == fom.TRUNCATED == model(orc, nonic_fixture, proof[:len(proof) - cut])
    assert library(p, nonic_fixture, proof + b"\0") == fom.LENGTH == model(orc, nonic_fixture, proof + b"\0")


def test_every_stark_kernel_compiles_without_scratch_and_the_committed_report_is_current():
    # The term program is indexed by loop counters and the accumulators are named registers, so no kernel may need scratch.  The compiler
    # is asked here (device code only, a few seconds, no GPU), and profiles/stark_resource_usage.txt must be what it answers: the
    # report is made by `make -s -C plonky2_demo_amd/csrc stark.resource_usage` and compared with the source positions left out.
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(GOLDEN))
    report = subprocess.run(["make", "-s", "-C", os.path.join(root, "plonky2_demo_amd", "csrc"), "stark.resource_usage"], capture_output=True, text=True, timeout=300)
    assert report.returncode == 0, report.stderr
    names = re.findall(r"Function Name: (\S+)", report.stdout)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", report.stdout)]
    assert len(names) == len(scratch) == 10 and not any(scratch), report.stdout
    with open(os.path.join(root, "plonky2_demo_amd", "csrc", "stark_kernels.cuh")) as f:
        declared = re.findall(r"__global__[^\n]*?void (k_\w+)", f.read())
    assert len(set(declared)) == 7 and all(any(k in n for n in names) for k in declared)
    with open(os.path.join(root, "profiles", "stark_resource_usage.txt")) as f:
        committed = f.read()
    unplaced = lambda text: re.sub(r"(?m)^\S+?:\d+:\d+: ", "", text)      # noqa: E731
    assert unplaced(committed) == unplaced(report.stdout), "profiles/stark_resource_usage.txt is stale"
