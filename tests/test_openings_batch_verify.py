"""The device batch verifier of FRI openings (gl_openings_batch_verifier: host stage per claim, Merkle paths and queries of a whole
batch on the device) against gl_verify_openings: for every claim of a call the same verdict and the same first failing check as
gl_verify_openings gives for that claim alone -- on valid STARK-shaped claims (one and two reductions, Keccak, a salted oracle), on
the tamper matrix of test_fri_openings.py at the first and the last query, on model-made proofs of arities 8 and 2, 4, across chunk
boundaries, host thread counts, reused staging and concurrent verifiers.  The tests at the end need no GPU."""
import ctypes
import threading

import numpy as np
import pytest

import fri_openings_model as fm
import prover_phase_model as pm
from oracle_lib import P
from test_fri_openings import EXACT, Layout, TinyProof, absorb, flip, library_challenger, stark_case, tamper_case
from transcript import poseidon_challenger
from vanishing_model import primitive_root

U64 = np.uint64
GL_ERR_ARG, GL_ERR_UNSUPPORTED, GL_ERR_VERIFY = 1, 3, 6


# ------------------------------------------------------------------------------- claims
class Claim:
    """one verify_fri_proof: what the host call and the batch call are both given"""

    def __init__(self, params, instance, caps, openings, proof, hasher="poseidon", points=None):
        self.params, self.instance, self.caps, self.openings, self.proof, self.hasher = params, instance, caps, openings, proof, hasher
        self.points = [pt for pt, _ in instance.batches] if points is None else points

    def host(self, p):
        """gl_verify_openings alone -> (accepted, message, code), or the refusal's code"""
        inst = p.FriInstance(self.instance.oracles, [(pt, polys) for pt, (_, polys) in zip(self.points, self.instance.batches)])
        try:
            return p.verify_fri_proof(inst, self.caps, self.openings, library_challenger(p, self.hasher, self.caps, self.openings), self.proof, self.params)
        except p.Plonky2Mi355xError as e:
            return e.code

    def batch(self, p):
        return (self.caps, self.openings, self.points, library_challenger(p, self.hasher, self.caps, self.openings), self.proof)


def of_case(case, proof=None, caps=None, openings=None, points=None):
    return Claim(case.params, case.instance, case.caps if caps is None else caps, case.openings if openings is None else openings,
                 case.proof if proof is None else proof, getattr(case, "hasher", "poseidon"), points)


def same(got, host):
    """the batch's (accepted, message, code) against the host's: the host's message carries the source position behind it"""
    assert not isinstance(host, int), host
    assert (got[0], got[2]) == (host[0], host[2]), (got, host)
    if host[0]:
        assert got[1] == "" and host[1] == "" and got[2] == 0
    else:
        assert got[1] and host[1].startswith(got[1] + " ("), (got, host)


def blank_instance(p, instance):
    """the instance with other points: the verifier ignores them"""
    return p.FriInstance(instance.oracles, [((3, 0), polys) for _, polys in instance.batches])


def verifier_of(gpu, case, **kw):
    p, ctx = gpu
    return p.OpeningsBatchVerifier(blank_instance(p, case.instance), case.params, ctx=ctx, **kw)


def run(gpu, bv, claims):
    """one batch call; every claim held against the host call"""
    p, ctx = gpu
    got = bv.verify([c.batch(p) for c in claims])
    assert len(got) == len(claims)
    for g, c in zip(got, claims):
        same(g, c.host(p))
    return got


# ------------------------------------------------------------------------------- 1. valid claims
@pytest.mark.gpu
@pytest.mark.parametrize("lg_n,hasher,kw,rounds", [(7, "poseidon", {}, 1), (11, "poseidon", {}, 2), (7, "keccak", {}, 1),
                                                    (7, "poseidon", dict(num_queries=6, blinding=(False, True, False)), 1)],
                         ids=["n128", "n2048", "keccak", "salted"])
def test_valid_claims_are_accepted_as_by_the_host(gpu, lg_n, hasher, kw, rounds):
    case = stark_case(gpu, lg_n, hasher, **kw)
    assert len(case.params.reduction_arity_bits) == rounds and bool(case.params.hiding) == bool(kw)
    got = run(gpu, verifier_of(gpu, case), [of_case(case)] * 3)
    assert got == [(True, "", 0)] * 3


# ------------------------------------------------------------------------------- 2. the tamper matrix
def transcript_mutants(case, lay):
    openings, caps = case.openings.copy(), case.caps.copy()
    openings[5, 1] ^= U64(1 << 9)
    caps[1, 3, 2] ^= U64(4)
    wrong_length = bytearray(case.proof)
    wrong_length[lay.sibling[0] - 1] += 1
    return [("opening value", of_case(case, openings=openings)), ("oracle cap", of_case(case, caps=caps)),
            ("commit cap", of_case(case, proof=flip(case.proof, lay.commit_caps + 40, bit=1))),
            ("final coefficient", of_case(case, proof=flip(case.proof, lay.final + 24, bit=1))),
            ("PoW witness", of_case(case, proof=flip(case.proof, lay.pow, bit=1))),
            ("truncated", of_case(case, proof=case.proof[:-1])), ("trailing byte", of_case(case, proof=case.proof + b"\0")),
            ("path-length byte", of_case(case, proof=bytes(wrong_length)))]


@pytest.mark.gpu
@pytest.mark.parametrize("lg_n", [7, 11])
def test_every_mutant_gets_the_hosts_verdict_and_first_failing_check(gpu, orc, lg_n):
    p, ctx = gpu
    case, lay, _ = tamper_case(gpu, orc, lg_n)
    xs, nq = case.trace["x_indices"], case.params.num_query_rounds
    mutants, want = [], {}
    for q in (0, nq - 1):
        for name, at_lg_n, where, code in EXACT:
            if at_lg_n == lg_n or (lg_n == 11 and name != "step sibling"):       # (the n = 2^11 proof takes the whole matrix, its step paths are not empty)
                at = where(lay, xs[q])
                assert lay.query0 < at < lay.query0 + lay.query_len
                mutants.append(("%s q%d" % (name, q), of_case(case, proof=flip(case.proof, at + q * lay.query_len, bit=3))))
                want[mutants[-1][0]] = code
    mutants += transcript_mutants(case, lay)
    # two faults in one proof: the earlier query's check is the one reported; inside a query the initial trees come first
    another_eval, leaf_word, at_x = EXACT[5][2], EXACT[1][2], EXACT[4][2]
    two = flip(flip(case.proof, another_eval(lay, xs[2]) + 2 * lay.query_len, bit=3), leaf_word(lay, xs[5]) + 5 * lay.query_len, bit=3)
    mutants.append(("step leaf in query 2 (the final polynomial would fail as well), leaf word in query 5", of_case(case, proof=two)))
    want[mutants[-1][0]] = fm.STEP_MERKLE
    one_query = flip(flip(case.proof, leaf_word(lay, xs[3]) + 3 * lay.query_len, bit=3), at_x(lay, xs[3]) + 3 * lay.query_len, bit=3)
    mutants.append(("leaf word of oracle 1 and evals[x & 15] in query 3", of_case(case, proof=one_query)))
    want[mutants[-1][0]] = fm.INITIAL_MERKLE
    claims = []
    for _, bad in mutants:                                # one call, the mutants between valid claims
        claims += [of_case(case), bad]
    got = run(gpu, verifier_of(gpu, case, max_batch=64, host_threads=2), claims)
    for k, (name, _) in enumerate(mutants):
        assert got[2 * k] == (True, "", 0), name
        assert not got[2 * k + 1][0], name
        if name in want:
            assert got[2 * k + 1][2] == want[name], (name, got[2 * k + 1])
    codes = {got[2 * k + 1][2] for k in range(len(mutants))}
    assert {fm.INITIAL_MERKLE, fm.FRI_CONSISTENCY, fm.STEP_MERKLE, fm.TRUNCATED, fm.LENGTH} <= codes


# ------------------------------------------------------------------------------- 3. arities other than 16: proofs from a model
def _rev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def _eval(coeffs, x):
    """Horner over extension coefficients at a base-field point"""
    a = b = 0
    for c0, c1 in reversed(coeffs):
        a, b = (a * x + c0) % P, (b * x + c1) % P
    return (a, b)


class ModelProof:
    """A FriProof written from the models (fri_openings_model.final_poly, prover_phase_model.fold) and the oracle's hash_or_noop /
    two_to_one: one oracle of two non-constant polynomials, n = 8, rate_bits 1, cap_height 1, no proof of work, 4 queries, any
    reduction arities.  A codeword is the list of its values at shift * w^rev(i), as the prover keeps it."""
    LG_N, RATE_BITS, CAP_HEIGHT, QUERIES = 3, 1, 1, 4

    def __init__(self, p, orc, arity_bits):
        self.p, self.hasher = p, "poseidon"
        self.params = p.FriParams(self.LG_N, self.RATE_BITS, self.CAP_HEIGHT, 0, self.QUERIES, arity_bits)
        point = (0x123456789, 0xFEDCBA987)
        self.instance = p.FriInstance([(2, False)], [(point, [(0, 0), (0, 1)])])
        n, lgN = 1 << self.LG_N, self.LG_N + self.RATE_BITS
        cols = [[(3 * k * k + 5 * k + 1 + 11 * c) * 0x9E3779B97F4A7C15 % P for k in range(n)] for c in range(2)]
        wN = primitive_root(lgN)
        xs = [7 * pow(wN, _rev(i, lgN), P) % P for i in range(1 << lgN)]
        leaves = [[_eval([(c, 0) for c in col], x)[0] for col in cols] for x in xs]
        levels = self.tree(orc, leaves)
        self.caps = np.array([levels[-1]], dtype=U64)
        self.openings = np.array(fm.openings_of(self.instance, [cols]), dtype=U64)
        ch = absorb(poseidon_challenger(orc), self.caps, self.openings)
        coeffs = fm.final_poly(self.instance, [cols], ch.get(2))
        words = lambda a: np.ascontiguousarray(np.asarray(a, dtype="<u8")).tobytes()      # noqa: E731
        out, shift, lg, steps = b"", 7, lgN, []
        for ab in arity_bits:
            w = primitive_root(lg)
            values = [_eval(coeffs, shift * pow(w, _rev(i, lg), P) % P) for i in range(1 << lg)]
            step_leaves = [[v for e in values[k << ab:(k + 1) << ab] for v in e] for k in range(1 << (lg - ab))]
            step_levels = self.tree(orc, step_leaves)
            steps.append((step_leaves, step_levels))
            out += words(step_levels[-1])
            ch.observe_hashes(np.array(step_levels[-1], dtype=U64))
            coeffs = pm.fold(coeffs, 1 << ab, ch.get(2))
            shift, lg = pow(shift, 1 << ab, P), lg - ab
        final = [v for c in coeffs for v in c]
        ch.observe(np.array(final, dtype=U64))
        ch.observe([0])
        ch.get(1)                                         # the proof-of-work response: no bits asked for
        self.x_index = [ch.get(1)[0] % (1 << lgN) for _ in range(self.QUERIES)]
        for x in self.x_index:
            out += words(leaves[x]) + self.path(levels, x)
            for ab, (step_leaves, step_levels) in zip(arity_bits, steps):
                x >>= ab
                out += words(step_leaves[x]) + self.path(step_levels, x)
        self.proof = out + words(final) + words([0])

    def tree(self, orc, leaves):
        """the levels from the leaf digests up to the cap"""
        levels = [[orc.hash_or_noop(np.array(leaf, dtype=U64)) for leaf in leaves]]
        while len(levels[-1]) > 1 << self.CAP_HEIGHT:
            below = levels[-1]
            levels.append([orc.two_to_one(below[2 * k], below[2 * k + 1]) for k in range(len(below) // 2)])
        return levels

    @staticmethod
    def path(levels, index):
        sib = b""
        for level in levels[:-1]:
            sib += np.ascontiguousarray(np.asarray(level[index ^ 1], dtype="<u8")).tobytes()
            index >>= 1
        return bytes([len(levels) - 1]) + sib

    def model(self, orc, proof):
        return fm.verify(self.params, self.instance, self.caps, self.openings, absorb(poseidon_challenger(orc), self.caps, self.openings), proof,
                         fm.poseidon_verify_path(orc))

    def mutants(self):
        """(name, proof, code): a leaf word, evals[within], another eval, a final coefficient -- in the last query where it matters"""
        lay, q = Layout(self.params, self.instance), self.QUERIES - 1
        ab, x, at = self.params.reduction_arity_bits[0], self.x_index[q], q * lay.query_len
        within = x & ((1 << ab) - 1)
        return [("leaf word", flip(self.proof, at + lay.leaf[0] + 8, 2), fm.INITIAL_MERKLE),
                ("evals[within]", flip(self.proof, at + lay.step_evals[0] + 16 * within, 2), fm.FRI_CONSISTENCY),
                ("another eval", flip(self.proof, at + lay.step_evals[0] + 16 * (within ^ 1) + 8, 2), fm.STEP_MERKLE),
                ("final coefficient", flip(self.proof, lay.final, 2), None)]      # (it moves the query indices: whatever both say)


_models = {}


def model_proof(orc, arity_bits):
    import plonky2_demo_amd as p
    if arity_bits not in _models:
        _models[arity_bits] = ModelProof(p, orc, list(arity_bits))
    return _models[arity_bits]


@pytest.mark.parametrize("arity_bits", [(3,), (1, 2)])
def test_model_made_proofs_of_other_arities_on_the_host(orc, arity_bits):
    import plonky2_demo_amd as p
    m = model_proof(orc, arity_bits)
    assert len(m.proof) == Layout(m.params, m.instance).size and len(set(m.x_index)) > 1
    assert m.model(orc, m.proof) == fm.ACCEPTED and of_case(m).host(p) == (True, "", 0)
    for name, bad, code in m.mutants():
        ok, why, got = of_case(m, proof=bad).host(p)
        assert not ok and got == m.model(orc, bad) != fm.ACCEPTED and code in (None, got), (name, got)


@pytest.mark.gpu
@pytest.mark.parametrize("arity_bits", [(3,), (1, 2)])
def test_model_made_proofs_of_other_arities_on_the_device(gpu, orc, arity_bits):
    p, ctx = gpu
    m = model_proof(orc, arity_bits)
    claims = [of_case(m)] + [of_case(m, proof=bad) for _, bad, _ in m.mutants()] + [of_case(m)]
    got = run(gpu, verifier_of(gpu, m, max_batch=8), claims)
    assert got[0] == got[-1] == (True, "", 0)
    for g, (name, _, code) in zip(got[1:], m.mutants()):
        assert not g[0] and code in (None, g[2]), (name, g)
    if arity_bits == (3,):                                # all zeros beside it: the same params
        t = TinyProof(p, orc)
        assert run(gpu, verifier_of(gpu, t), [of_case(t), of_case(t, proof=flip(t.proof, Layout(t.params, t.instance).leaf[0]))])[0] == (True, "", 0)


# ------------------------------------------------------------------------------- 4. a non-canonical leaf word, a point on the coset
@pytest.mark.gpu
def test_a_non_canonical_leaf_word_is_accepted_as_by_the_host(gpu, orc):
    # the host takes every word mod p, and so does the table the device reads: w < 2^32 - 1 written as w + p still fits 64 bits
    p, ctx = gpu
    t = TinyProof(p, orc)
    at = Layout(t.params, t.instance).leaf[0]
    w = int.from_bytes(t.proof[at:at + 8], "little")
    assert w < 2**32 - 1
    bad = t.proof[:at] + (w + P).to_bytes(8, "little") + t.proof[at + 8:]
    assert bad != t.proof and of_case(t, proof=bad).host(p) == (True, "", 0)
    assert run(gpu, verifier_of(gpu, t), [of_case(t), of_case(t, proof=bad)]) == [(True, "", 0)] * 2


@pytest.mark.gpu
def test_a_claim_whose_point_lies_on_the_coset_is_refused_alone(gpu, orc):
    p, ctx = gpu
    case = stark_case(gpu, 7, num_queries=6, blinding=(False, True, False))
    lay = Layout(case.params, case.instance)
    on_coset = (7 * pow(primitive_root(8), 5, P) % P, 0)
    refused = of_case(case, points=[case.instance.batches[0][0], on_coset])
    assert refused.host(p) == GL_ERR_ARG
    claims = [of_case(case), refused, of_case(case, proof=flip(case.proof, lay.leaf[0])), of_case(case)]
    bv = verifier_of(gpu, case)
    with pytest.raises(p.Plonky2Mi355xError) as e:
        bv.verify([c.batch(p) for c in claims])
    assert e.value.code == GL_ERR_ARG
    assert bv.verdicts == [0, GL_ERR_ARG, GL_ERR_VERIFY, 0] and bv.checks == [0, 0, fm.INITIAL_MERKLE, 0]


# ------------------------------------------------------------------------------- 5. batch mechanics
def good_and_bad(case):
    lay = Layout(case.params, case.instance)
    last = (case.params.num_query_rounds - 1) * lay.query_len
    bad = [of_case(case, proof=flip(case.proof, at)) for at in (lay.leaf[0], lay.sibling[1] + 8, lay.step_evals[0] + last, lay.leaf[2] + last, lay.pow)]
    return of_case(case), bad + [of_case(case, proof=case.proof[:-1])]


@pytest.mark.gpu
def test_counts_chunks_threads_and_reused_staging(gpu):
    p, ctx = gpu
    case = stark_case(gpu, 7, num_queries=6, blinding=(False, True, False))
    good, bad = good_and_bad(case)
    host = {id(c): c.host(p) for c in [good] + bad}
    assert host[id(good)][0] and not any(host[id(c)][0] for c in bad)
    one, four = verifier_of(gpu, case, max_batch=4, host_threads=1), verifier_of(gpu, case, max_batch=4, host_threads=4)
    pattern = [good, bad[0], good, bad[1], bad[2], good, bad[3], bad[4], good, good, bad[5]]       # bad claims on both sides of a chunk boundary
    for count in (0, 1, 4, 5, 11):
        claims = pattern[:count]
        a, b = one.verify([c.batch(p) for c in claims]), four.verify([c.batch(p) for c in claims])
        assert a == b and len(a) == count and one.checks == four.checks
        for g, c in zip(a, claims):
            same(g, host[id(c)])
    # stale flags: after a batch full of rejections the same verifier accepts a good batch
    assert not any(ok for ok, _, _ in one.verify([c.batch(p) for c in bad[:4]]))
    assert one.verify([good.batch(p) for _ in range(4)]) == [(True, "", 0)] * 4
    # checks = NULL and count = 0 are accepted
    lib = p._lib.lib
    assert lib.gl_openings_batch_verifier_verify(one.handle, None, 0, None, None) == 0
    caps, openings, points, ch, proof = good.batch(p)
    pts, buf = np.array(points, dtype=U64), np.frombuffer(proof, dtype=np.uint8)
    claim = p._lib.OpeningsClaim(caps.ctypes.data, openings.ctypes.data, pts.ctypes.data, ch.handle, buf.ctypes.data, buf.size)
    verdict = np.full(1, -1, dtype=np.int32)
    assert lib.gl_openings_batch_verifier_verify(one.handle, ctypes.byref(claim), 1, verdict.ctypes.data_as(ctypes.c_void_p), None) == 0 and verdict[0] == 0
    claim.caps = None                                     # a null inside a claim is a failure of the call, not a verdict
    assert lib.gl_openings_batch_verifier_verify(one.handle, ctypes.byref(claim), 1, verdict.ctypes.data_as(ctypes.c_void_p), None) == GL_ERR_ARG


@pytest.mark.gpu
def test_two_verifiers_on_two_contexts_from_two_threads(gpu):
    p, ctx = gpu
    case = stark_case(gpu, 7, num_queries=6, blinding=(False, True, False))
    good, bad = good_and_bad(case)
    batches = [[good, bad[0], bad[3], good, bad[5], bad[1]] * 3, [bad[2], good, bad[4], bad[1]] * 4]
    bvs = [p.OpeningsBatchVerifier(blank_instance(p, case.instance), case.params, ctx=p.Context(0), max_batch=8, host_threads=2) for _ in batches]
    want = [bv.verify([c.batch(p) for c in b]) for bv, b in zip(bvs, batches)]
    for answers, b in zip(want, batches):
        for g, c in zip(answers, b):
            same(g, c.host(p))
    got, errors = [None] * len(bvs), []

    def work(k):
        try:
            for _ in range(3):
                got[k] = bvs[k].verify([c.batch(p) for c in batches[k]])
        except Exception as e:                            # noqa: BLE001  (re-raised below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(bvs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    assert got == want


# ------------------------------------------------------------------------------- 6. no GPU needed
NEW_SYMBOLS = ("gl_openings_batch_verifier_new", "gl_openings_batch_verifier_verify", "gl_openings_batch_verifier_free")


def test_the_symbols_are_declared_exported_and_bound():
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    from test_abi import declared_symbols
    declared = declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert p.OpeningsBatchVerifier is p.api.OpeningsBatchVerifier


def test_new_refuses_null_arguments_limits_and_arity_32():
    import plonky2_demo_amd as p
    from plonky2_demo_amd._lib import lib
    params, inst = p.FriParams(7, 1, 4, 16, 84, [4]), p.FriInstance([(1, False)], [((5, 0), [(0, 0)])])
    not_a_context = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)      # the argument checks come before anything reads the context
    h = ctypes.c_void_p()
    new = lib.gl_openings_batch_verifier_new
    assert new(None, ctypes.byref(params), ctypes.byref(inst), 4, 1, ctypes.byref(h)) == GL_ERR_ARG and not h.value
    assert new(not_a_context, None, ctypes.byref(inst), 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    assert new(not_a_context, ctypes.byref(params), None, 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    assert new(not_a_context, ctypes.byref(params), ctypes.byref(inst), 4, 1, None) == GL_ERR_ARG
    for max_batch in (0, 4097):
        assert new(not_a_context, ctypes.byref(params), ctypes.byref(inst), max_batch, 1, ctypes.byref(h)) == GL_ERR_ARG
        assert b"max_batch" in lib.gl_last_error() and not h.value
    assert new(not_a_context, ctypes.byref(params), ctypes.byref(inst), 4, 65, ctypes.byref(h)) == GL_ERR_ARG
    # what glfri::check refuses, with its code; then the one refusal of the device path's own
    assert new(not_a_context, ctypes.byref(p.FriParams(7, 1, 4, 16, 0, [4])), ctypes.byref(inst), 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    assert b"query rounds" in lib.gl_last_error()
    assert new(not_a_context, ctypes.byref(p.FriParams(7, 1, 2, 16, 84, [5])), ctypes.byref(inst), 4, 1, ctypes.byref(h)) == GL_ERR_UNSUPPORTED and not h.value
    lib.gl_openings_batch_verifier_free(None)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import plonky2_demo_amd as p
    with pytest.raises(p.Plonky2Mi355xError):
        p.OpeningsBatchVerifier(p.FriInstance([(1, False)], [((5, 0), [(0, 0)])]), p.FriParams(7, 1, 4, 16, 84, [4]))
