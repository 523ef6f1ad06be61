"""CPU tests of the table-set host code (csrc/stark_set.hip, csrc/host_api.hip): gl_stark_set_check's refusals, each beside the boundary
case it accepts, the Z counts it derives, and gl_challenger_compact against the model under both hashers."""
import ctypes

import numpy as np
import pytest

import stark_ctl_airs as airs
import stark_ctl_model as cm
from stark_airs import ALL, LOCAL
from stark_ctl_airs import single, twc

ARG, UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def p():
    import plonky2_demo_amd
    return plonky2_demo_amd


def table(p, columns=4, degree=3, pairs=(), challenges=2):
    return p.StarkDesc(columns, 0, degree, [(ALL, [(1, [(LOCAL, 0)])])], pairs).struct(challenges)


def params(p, degree_bits=5, rate_bits=1, cap_height=4, pow_bits=16, queries=84, arity=None, hasher="poseidon"):
    if arity is None:                                        # ConstantArityBits(4, 5)
        arity, d = [], degree_bits
        while d > 5 and d + rate_bits - 4 >= cap_height:
            arity, d = arity + [4], d - 4
    return p.FriParams(degree_bits, rate_bits, cap_height, pow_bits, queries, arity, False, hasher)


def flat(lookups):
    return [([(t.table, t.columns, t.filter) for t in looking], (looked.table, looked.columns, looked.filter)) for looking, looked in lookups]


def status(p, tables=None, lookups=None, tweak=None, verifier=False):
    """gl_stark_set_check -> (status, message); the default is an accepted set of two tables and one filtered lookup.  verifier: the same
    validation as the host-only entries run it (gl_stark_set_num_zs), which take FRI arity bits 1..8 where the prover takes 4 only"""
    tables = [(table(p), params(p)), (table(p), params(p, 6))] if tables is None else tables
    lookups = [([twc(0, [single(0), single(1)], single(2))], twc(1, [single(0), single(1)], single(3)))] if lookups is None else lookups
    st = p.api._lib.StarkSetDescStruct(tables, flat(lookups))
    if tweak:
        tweak(st)
    rc = p.api.lib.gl_stark_set_num_zs(ctypes.byref(st), 0, None, None) if verifier else p.api.lib.gl_stark_set_check(ctypes.byref(st))
    return rc, (p.api.lib.gl_last_error() or b"").decode() if rc else ""


def with_pair(p, k, **kw):
    return [(table(p, pairs=[[(0, 1)]]), params(p, **kw)) for _ in range(k)]


def lookup_of(looking, looked, ncols=2, filt=None):
    return ([twc(t, [single(c) for c in range(ncols)], filt) for t in looking], twc(looked, [single(c) for c in range(ncols)], filt))


def set_field(name, value):
    def tweak(st):
        setattr(st, name, value)
    return tweak


def test_the_default_set_is_accepted(p):
    assert status(p) == (0, "")


def cases(p):
    two = lambda **kw: [(table(p), params(p)), (table(p), params(p, **kw))]                            # noqa: E731
    wide = [(table(p, columns=70), params(p)), (table(p, columns=70), params(p))]
    col = lambda k: ([(c, 1) for c in range(k)], 0)                                                    # noqa: E731
    return [
        # (what, refused keywords, message fragment, accepted keywords)
        ("no tables", dict(tables=[]), "1..8 tables", dict(tables=with_pair(p, 1), lookups=[])),
        ("nine tables", dict(tables=with_pair(p, 9), lookups=[]), "1..8 tables", dict(tables=with_pair(p, 8), lookups=[])),
        ("a table's own description", dict(tables=[(table(p, columns=0), params(p)), (table(p), params(p))]), "columns", dict()),
        ("another hasher", dict(tables=two(hasher="keccak")), "must agree", dict(tables=two(degree_bits=7))),
        ("another rate", dict(tables=two(rate_bits=2)), "must agree", dict()),
        ("another cap height", dict(tables=two(cap_height=3)), "must agree", dict()),
        ("another query count", dict(tables=two(queries=83)), "must agree", dict()),
        ("other proof-of-work bits", dict(tables=two(pow_bits=15)), "must agree", dict()),
        ("another num_challenges", dict(tables=[(table(p), params(p)), (table(p, challenges=1), params(p))]), "must agree", dict()),
        ("another reduction strategy", dict(verifier=True, tables=[(table(p), params(p, 8, arity=[3])), (table(p), params(p, 8, arity=[2]))]), "one arity",
         dict(verifier=True, tables=[(table(p), params(p, 8, arity=[3])), (table(p), params(p, 12, arity=[3, 3]))])),
        ("a filter with q = 1", dict(tables=[(table(p, degree=2), params(p)), (table(p), params(p))]), "constraint_degree >= 3",
         dict(tables=[(table(p, degree=3), params(p)), (table(p), params(p))])),
        ("a filter with q = 1 on the looked table", dict(tables=[(table(p), params(p)), (table(p, degree=2), params(p))]), "constraint_degree >= 3", dict()),
        ("no filter with q = 1 (accepted) / degree 1 too", dict(tables=[(table(p, degree=2), params(p)), (table(p, degree=2), params(p))]), "constraint_degree >= 3",
         dict(tables=[(table(p, degree=2), params(p)), (table(p, degree=1), params(p))], lookups=[lookup_of([0], 1)])),
        ("mismatched column counts", dict(lookups=[([twc(0, [single(0), single(1)])], twc(1, [single(0)]))]), "number of columns",
         dict(lookups=[([twc(0, [single(0)])], twc(1, [single(0)]))])),
        ("a table without Zs", dict(tables=[(table(p), params(p))] * 3), "No CTL?", dict(tables=[(table(p), params(p))] * 2 + with_pair(p, 1))),
        ("a duplicate column in a combination", dict(lookups=[([twc(0, [([(1, 2), (1, 3)], 0)])], twc(1, [single(0)]))]), "duplicate columns",
         dict(lookups=[([twc(0, [([(1, 2), (2, 3)], 0)])], twc(1, [single(0)]))])),
        ("65 terms", dict(tables=wide, lookups=[([twc(0, [col(65)])], twc(1, [single(0)]))]), "64 terms",
         dict(tables=wide, lookups=[([twc(0, [col(64)])], twc(1, [single(0)]))])),
        ("17 columns", dict(tables=wide, lookups=[lookup_of([0], 1, 17)]), "1..16 columns", dict(tables=wide, lookups=[lookup_of([0], 1, 16)])),
        ("no columns", dict(lookups=[lookup_of([0], 1, 0)]), "1..16 columns", dict(lookups=[lookup_of([0], 1, 1)])),
        ("nine looking tables", dict(lookups=[lookup_of([0] * 9, 1)]), "1..8 looking", dict(lookups=[lookup_of([0] * 8, 1)])),
        ("no looking table", dict(lookups=[lookup_of([], 1)]), "1..8 looking", dict(lookups=[lookup_of([0], 1)])),
        ("33 lookups", dict(lookups=[lookup_of([0], 1)] * 33), "32 cross-table lookups", dict(lookups=[lookup_of([0], 1)] * 32)),
        ("a table index out of range", dict(lookups=[lookup_of([0], 2)]), "table index", dict(lookups=[lookup_of([0], 1)])),
        ("a trace column out of range", dict(lookups=[([twc(0, [single(4)])], twc(1, [single(0)]))]), "trace column is out of range",
         dict(lookups=[([twc(0, [single(3)])], twc(1, [single(0)]))])),
        ("a filter column out of range", dict(lookups=[([twc(0, [single(0)], single(4))], twc(1, [single(0)]))]), "trace column is out of range", dict()),
        ("a TableWithColumns left over", dict(tweak=set_field("num_twcs", 3)), "exactly", dict()),
        ("a TableWithColumns short", dict(tweak=set_field("num_twcs", 1)), "more TableWithColumns than the pool", dict()),
        ("a Column left over", dict(tweak=set_field("num_ctl_columns", 7)), "exactly", dict()),
        ("a Column short", dict(tweak=set_field("num_ctl_columns", 5)), "more Columns than the pool", dict()),
        ("a null pool", dict(tweak=set_field("twc_table", None)), "null lookup table", dict()),
        ("null tables", dict(tweak=set_field("tables", None)), "null tables", dict()),
    ]


def test_every_refusal_beside_the_case_it_accepts(p):
    for what, refused, fragment, accepted in cases(p):
        rc, msg = status(p, **refused)
        assert rc == ARG and fragment in msg, "%s: status %d, %r" % (what, rc, msg)
        assert status(p, **accepted) == (0, ""), "%s: the accepted neighbour is refused: %r" % (what, status(p, **accepted))


def test_a_null_description_and_a_table_refusal_that_is_unsupported(p):
    assert p.api.lib.gl_stark_set_check(None) == ARG
    rc, msg = status(p, tables=[(table(p, degree=4), params(p)), (table(p), params(p))])              # degree above the rate: gl_stark_check's own
    assert rc == UNSUPPORTED and "higher than the rate" in msg


@pytest.mark.parametrize("nc", [1, 2])
def test_the_z_counts_are_the_reference_s(p, nc):
    # num_ctl_zs (cross_table_lookup.rs:178-185) and num_permutation_batches (stark.rs:216-221) of the test system; a table may be looking
    # and looked (mul), stand in several lookups (ops) and twice in one
    desc = airs.api_set(p, airs.TABLES, airs.LOOKUPS, [5, 6, 5], airs.config(p, nc))
    desc.check()
    assert [desc.num_zs(t) for t in range(3)] == [(0, 2 * nc), (-(-nc // 2), nc), (0, 2 * nc)]
    assert [cm.num_ctl_zs(airs.LOOKUPS, t, nc) for t in range(3)] == [2 * nc, nc, 2 * nc]
    twice = airs.LOOKUPS + [([twc(airs.OPS, [single(0)]), twc(airs.OPS, [single(1)])], twc(airs.OPS, [single(2)]))]
    desc = airs.api_set(p, airs.TABLES, twice, [5, 6, 5], airs.config(p, nc))
    assert desc.num_zs(airs.OPS) == (0, 5 * nc) and cm.num_ctl_zs(twice, airs.OPS, nc) == 5 * nc
    with pytest.raises(p.Plonky2Mi355xError, match="table index"):
        desc.num_zs(3)


def test_python_columns_are_the_reference_s_constructors(p):
    C = p.CtlColumn
    assert C.single(3).flat() == ([(3, 1)], 0) and C.constant(9).flat() == ([], 9)
    assert C.le_bits([4, 5, 6]).flat() == ([(4, 1), (5, 2), (6, 4)], 0) and C.sum([1, 2]).flat() == ([(1, 1), (2, 1)], 0)
    assert C.linear_combination([(8, 3)], 7).flat() == ([(8, 3)], 7)
    with pytest.raises(ValueError):
        C.linear_combination([])


# ------------------------------------------------------------------------------- Challenger::compact
def challengers(p, orc, hasher):
    if hasher == "poseidon":
        return p.Challenger(), cm.poseidon_challenger(orc)
    import test_keccak
    return p.Challenger(hasher="keccak"), cm.CompactChallenger(test_keccak.model_permute, test_keccak.model_hash_elements)


@pytest.mark.parametrize("hasher", ["poseidon", "keccak"])
def test_compact_matches_the_model(p, orc, hasher):
    # pending input -> one duplexing; a non-empty output buffer -> dropped, so the next challenge costs a permutation; both empty -> the
    # state stays, the next challenge still permutes
    ch, mo = challengers(p, orc, hasher)
    rng = np.random.default_rng(7)
    seen = set()
    ch.compact()                                             # both buffers empty
    mo.compact()
    assert ch.get_n_challenges(2) == mo.get(2)
    for step in range(40):
        xs = rng.integers(0, 2**64, int(rng.integers(0, 11)), dtype=np.uint64)
        ch.observe_elements(xs)
        mo.observe(xs)
        k = int(rng.integers(0, 4))
        assert ch.get_n_challenges(k) == mo.get(k)
        if step % 2:
            seen.add((bool(mo.inp), bool(mo.out)))
            ch.compact()
            mo.compact()
            assert not mo.inp and not mo.out
            st, buf = ch.state()
            assert [int(x) % cm.P for x in st] == [x % cm.P for x in mo.state] and len(buf) == 0
        assert ch.get_n_challenges(1) == mo.get(1)
    assert {(True, False), (False, True)} <= seen


def test_compact_changes_the_next_challenge(p):
    a, b = p.Challenger(), p.Challenger()
    for c in (a, b):
        c.observe_elements([1, 2, 3])
        c.get_n_challenges(1)
    b.compact()
    assert a.get_n_challenges(1) != b.get_n_challenges(1)
    assert p.api.lib.gl_challenger_compact(None) == ARG


# ------------------------------------------------------------------------------- the committed set proof
import json  # noqa: E402
import os  # noqa: E402

import fri_openings_model as fom  # noqa: E402
import stark_model as sm  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fixture(p):
    with open(os.path.join(GOLDEN, "stark_ctl_set.bin"), "rb") as f:
        proof = f.read()
    with open(os.path.join(GOLDEN, "stark_ctl_set.json")) as f:
        meta = json.load(f)
    desc = airs.api_set(p, airs.TABLES, airs.LOOKUPS, meta["degree_bits"], airs.config(p, meta["num_challenges"]))
    return proof, meta, desc, [desc.fri_params(t) for t in range(3)]


def library(p, fixture, proof):
    ok, why, code, table = p.stark_set_verify(fixture[2], proof)
    assert ok == (code == 0)
    return code, table


def model(orc, fixture, proof):
    return cm.verify_set(airs.TABLES, airs.LOOKUPS, fixture[1]["num_challenges"], fixture[3], proof, cm.poseidon_challenger(orc), fom.poseidon_verify_path(orc))


def regions(fixture):
    """byte offset of every region of every table's proof: {(table, name): (first byte, length)}"""
    _, meta, _, params = fixture
    nc, out, pos = meta["num_challenges"], {}, 0
    for t, (air, p_) in enumerate(zip(airs.TABLES, params)):
        cap, nctl = 32 << p_.cap_height, meta["num_ctl_zs"][t]
        nzs = meta["num_permutation_zs"][t] + nctl
        for name, size in (("trace_cap", cap), ("zs_cap", cap), ("quotient_cap", cap), ("local", 16 * air.num_columns), ("next", 16 * air.num_columns), ("zs", 16 * nzs),
                           ("zs_next", 16 * nzs), ("ctl_zs_last", 8 * nctl), ("quotient", 16 * air.q * nc)):
            out[t, name] = (pos, size)
            pos += size
        end = out[t, "trace_cap"][0] + cm.table_proof_size(air, nc, nctl, p_)
        out[t, "fri"] = (pos, end - pos)
        out[t, "all"] = (out[t, "trace_cap"][0], end - out[t, "trace_cap"][0])
        pos = end
    return out


def test_both_verifiers_accept_the_committed_set_proof(p, orc, fixture):
    proof, meta = fixture[:2]
    assert len(proof) == meta["num_bytes"] == sum(size for (_, name), (_, size) in regions(fixture).items() if name == "all")
    assert library(p, fixture, proof) == (0, 3) == model(orc, fixture, proof)
    assert cm.check_ctls(airs.traces(meta["degree_bits"], seed=meta["trace_seed"]), airs.LOOKUPS)


FRI_CHECKS = (fom.POW, fom.INITIAL_MERKLE, fom.FRI_CONSISTENCY, fom.STEP_MERKLE, fom.FINAL_POLY)


def test_the_tamper_matrix(p, orc, fixture):
    # one flipped bit per row; the documented order decides what answers it.  (table, region, word) -> the check and the table reported;
    # a tuple of checks = "one of the FRI checks", where the transcript the change feeds decides which (the model must name the same)
    proof, reg = fixture[0], regions(fixture)
    rows = [
        # ctl_zs_last of a looking table: its table's batch at g^-1 no longer opens the committed Z, and the word feeds the FRI challenges;
        # the FRI checks of that table come before the cross-table product, which would fail too
        ((airs.OPS, "ctl_zs_last", 0), FRI_CHECKS, airs.OPS),
        ((airs.OPS2, "ctl_zs_last", 1), FRI_CHECKS, airs.OPS2),
        ((airs.OPS2, "zs", 0), sm.VANISHING, airs.OPS2),             # the permutation Z's opening
        ((airs.OPS2, "zs", 2), sm.VANISHING, airs.OPS2),             # a CTL Z's opening
        ((airs.MUL, "zs_next", 3), sm.VANISHING, airs.MUL),
        ((airs.MUL, "local", 0), sm.VANISHING, airs.MUL),
        ((airs.MUL, "trace_cap", 0), sm.VANISHING, airs.OPS),        # every trace cap is observed first: the CTL challenges change for table 0 already
        ((airs.OPS2, "zs_cap", 0), sm.VANISHING, airs.OPS2),         # its alphas change
        ((airs.OPS, "quotient_cap", 0), sm.VANISHING, airs.OPS),     # its zeta changes
        ((airs.MUL, "fri", 40), FRI_CHECKS, airs.MUL),
    ]
    for (table, name, word), check, reported in rows:
        bad = bytearray(proof)
        bad[reg[table, name][0] + 8 * word] ^= 1
        got = library(p, fixture, bytes(bad))
        assert got == model(orc, fixture, bytes(bad)), (table, name, word, got)
        assert got[1] == reported and (got[0] in check if isinstance(check, tuple) else got[0] == check), (table, name, word, got)


def test_a_flipped_ctl_zs_last_word_of_every_table(p, orc, fixture):
    # the words the per-table stage hands to the product across the tables: the last word of each table's, the looked table's among them
    # (the matrix above holds ops' first and ops2's second).  The table's own batch at g^-1 answers, before the product check.
    proof, meta, reg = fixture[0], fixture[1], regions(fixture)
    for table in (airs.OPS, airs.OPS2, airs.MUL):
        first, size = reg[table, "ctl_zs_last"]
        assert size == 8 * meta["num_ctl_zs"][table] > 0
        bad = bytearray(proof)
        bad[first + size - 8] ^= 1
        got = library(p, fixture, bytes(bad))
        assert got == model(orc, fixture, bytes(bad)), (table, got)
        assert got[0] in FRI_CHECKS and got[1] == table, (table, got)


def test_swapped_tables_and_truncation(p, orc, fixture):
    proof, reg = fixture[0], regions(fixture)
    (a0, al), (b0, bl), (c0, cl) = reg[airs.OPS, "all"], reg[airs.OPS2, "all"], reg[airs.MUL, "all"]
    swapped = proof[c0:c0 + cl] + proof[b0:b0 + bl] + proof[a0:a0 + al]          # the same length, ops and mul in each other's place
    got = library(p, fixture, swapped)
    assert got == model(orc, fixture, swapped) and got[0] != 0 and got[1] == airs.OPS
    for cut in (1, 8, len(proof) - 100, len(proof)):
        assert library(p, fixture, proof[:len(proof) - cut]) == (fom.TRUNCATED, 3) == model(orc, fixture, proof[:len(proof) - cut])
    assert library(p, fixture, proof + b"\0") == (fom.LENGTH, 3) == model(orc, fixture, proof + b"\0")
