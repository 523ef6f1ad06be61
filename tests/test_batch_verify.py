"""The batch verifier (gl_batch_verifier: host stage per proof, Merkle paths and FRI queries of a whole batch on the device) against
gl_verify: for every proof of a call the same verdict and the same first failing check as gl_verify gives for that proof alone --
on valid proofs of every code path (0, 1 and 2 FRI rounds, lookups, salted leaves, Keccak, the extension gates), on a matrix of
mutants built with the proof parser, across chunk boundaries, host thread counts, reused staging and concurrent verifiers.
The tests at the end need no GPU: the symbols, the check texts, the argument checks."""
import ctypes
import threading

import numpy as np
import pytest

import ext_gate_circuits as egc
from oracle_lib import rand_field
from proof_mutants import _bump, _emit, _host_stage_mutants, _query_mutants, _non_canonical_leaf_word
from proof_parser import ParsedProof

U64 = np.uint64
_NO_PIS = np.zeros(0, dtype=U64)


def _same(batch, host):
    """(accepted, reason) of the batch verifier against CircuitData.verify's: the host's reason carries the source position behind it"""
    assert batch[0] == host[0], (batch, host)
    if host[0]:
        assert batch[1] == "" and host[1] == ""
    else:
        assert batch[1] and host[1].startswith(batch[1] + " ("), (batch, host)


# ------------------------------------------------------------------------------- circuits and their proofs
class _Case:
    """A circuit on the device, `proofs` of different witnesses with the Proof objects kept (their query indices)."""

    def __init__(self, cd, proofs):
        self.cd, self.desc = cd, cd.desc
        self.x_index = [pr.query_indices() for pr in proofs]
        self.proofs = [pr.to_bytes() for pr in proofs]


def _matmul_case(p, ctx, m, count=3, zk=False, hasher="poseidon"):
    hc = p.MatmulCircuit(m, zero_knowledge=zk, hasher=hasher)
    cd = hc.build(ctx)
    proofs = []
    for k in range(count):
        a, b = rand_field(70 + m + k, m * m) % (2**32 - 1), rand_field(170 + m + k, m * m) % (2**32 - 1)
        wires, pis = hc.witness(a, b, filler_seed=k)
        if zk:
            buf = ctx.alloc(wires.nbytes).upload(wires)
            cd.blind_witness(buf.ptr)
            proofs.append(cd.prove_device(buf.ptr, pis))
            buf.free()
        else:
            proofs.append(cd.prove(wires, pis))
    return _Case(cd, proofs)


def _two_round_m():
    """the matmul size of the two-round case: m = 20 if its circuit has 2^10 rows, else the smallest m that has"""
    import plonky2_demo_amd as p
    return next(m for m in range(20, 64) if p.MatmulCircuit(m).desc.degree_bits >= 10)


def _lookup_case(p, ctx, orc):
    oc = orc.circuit_of_kind(8, 2, threads=4)                        # lookup_test.rs test_one_lookup, as in test_gpu_parity.py
    cd = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas(), ctx)
    proofs = []
    for inputs in ([1, 2], [3, 4], [200, 7]):
        w = oc.witness(np.array(inputs, dtype=U64), _NO_PIS, filler_seed=2)
        proofs.append(cd.prove(w.wires(), w.public_inputs()))
    return _Case(cd, proofs)


def _chained_case(p, ctx):
    c = egc.Chained(seed=3, min_degree_bits=6).circuit
    cd = p.GenericCircuitData.from_classes(c.desc, c.constants, c.classes, ctx=ctx)
    return _Case(cd, [cd.prove(c.wires(), _NO_PIS) for _ in range(2)])       # (the circuit is its witness: the same proof twice)


_cases = {}


def _case(gpu, orc, name):
    """built once, shared, never changed"""
    if name not in _cases:
        p, ctx = gpu
        make = {
            "m2": lambda: _matmul_case(p, ctx, 2), "m8": lambda: _matmul_case(p, ctx, 8), "m20": lambda: _matmul_case(p, ctx, _two_round_m()),
            "lookup": lambda: _lookup_case(p, ctx, orc), "zk8": lambda: _matmul_case(p, ctx, 8, zk=True),
            "keccak8": lambda: _matmul_case(p, ctx, 8, hasher="keccak"), "chained": lambda: _chained_case(p, ctx),
        }
        _cases[name] = make[name]()
    return _cases[name]


# ------------------------------------------------------------------------------- 1. acceptance equals the host
@pytest.mark.gpu
@pytest.mark.parametrize("name,rounds", [("m2", 0), ("m8", 1), ("m20", 2), ("lookup", 0), ("zk8", 3), ("keccak8", 1), ("chained", 1)])
def test_valid_proofs_are_accepted_as_by_the_host(gpu, orc, name, rounds):
    c = _case(gpu, orc, name)
    d = c.desc
    assert d.num_fri_rounds == rounds                    # (the blinding rows of the zero-knowledge build take m = 8 to 2^14 rows: three rounds)
    assert d.degree_bits == {"m2": 3, "m8": 7}.get(name, d.degree_bits) and (name != "m20" or d.degree_bits >= 10)
    assert (d.num_lookup_polys > 0) == (name == "lookup") and d.zero_knowledge == (name == "zk8") and d.hasher == (name == "keccak8")
    bv = c.cd.batch_verifier()
    got = bv.verify(c.proofs)
    assert len(got) == len(c.proofs) >= 2
    for by, g in zip(c.proofs, got):
        assert g == (True, "")
        assert c.cd.verify(by) == (True, "")
    assert bv.checks == [0] * len(c.proofs)


# ------------------------------------------------------------------------------- 2. the tamper matrix
def _two_faults(d, by):
    pp = ParsedProof(d, by)
    h = pp.queries[5][1][0][1][0]                        # a step sibling at query 5 ...
    if d.hasher:
        h[0] ^= U64(1)
    else:
        _bump(h, 2)
    _bump(pp.queries[20][0][1][0], 1)                    # ... and an initial leaf at query 20
    return "two faults: step sibling at query 5, initial leaf at query 20", _emit(d, pp)


@pytest.mark.gpu
@pytest.mark.parametrize("name,whole", [("m8", True), ("m20", True), ("keccak8", False), ("zk8", False)])
def test_every_mutant_gets_the_hosts_verdict_and_first_failing_check(gpu, orc, name, whole):
    c = _case(gpu, orc, name)
    d, by, x_index = c.desc, c.proofs[0], c.x_index[0]
    assert d.num_query_rounds == 28 and _emit(d, ParsedProof(d, by)) == by
    mutants = _query_mutants(d, by, x_index, 0) + _query_mutants(d, by, x_index, 27)
    if whole:
        mutants += _host_stage_mutants(d, by) + [_two_faults(d, by)]
    batch = []
    for k, (_, bad) in enumerate(mutants):               # one call, the mutants between valid proofs
        batch += [c.proofs[k % len(c.proofs)], bad]
    bv = c.cd.batch_verifier(max_batch=64, host_threads=2)
    got = bv.verify(batch)
    reasons = {}
    for k, (what, bad) in enumerate(mutants):
        assert got[2 * k] == (True, "") and bv.checks[2 * k] == 0, what          # the valid neighbours
        host = c.cd.verify(bad)
        _same(got[2 * k + 1], host)
        assert (bv.checks[2 * k + 1] == 0) == host[0]
        assert host[0] == what.startswith("m:"), what
        reasons[what] = got[2 * k + 1][1]
    # the matrix reaches every check of the query phase, at the first and at the last query
    for q in (0, 27):
        assert reasons["d: initial leaf of tree 0 q%d" % q] == reasons["e: initial sibling, last level q%d" % q] == "initial Merkle proof fails"
        assert reasons["f: step leaf at x & 15, round 0 q%d" % q] == "FRI consistency check fails"
        assert reasons["g: another step leaf entry, round 0 q%d" % q] == reasons["h: step sibling, round 0 q%d" % q] == "FRI step Merkle proof fails"
    if whole:
        # (the final polynomial enters the transcript in front of the proof-of-work witness: changing it moves the response, and that
        # check comes first; the final-polynomial comparison itself is reached by no single change of a proof)
        assert reasons["i: final polynomial coefficient"] in ("invalid proof of work witness", "final polynomial evaluation is invalid")
        assert reasons["two faults: step sibling at query 5, initial leaf at query 20"] == "FRI step Merkle proof fails"
        assert reasons["a: opening word"].startswith("vanishing") and reasons["b: proof-of-work witness"] == "invalid proof of work witness"


@pytest.mark.gpu
def test_a_non_canonical_leaf_word_is_accepted_as_by_the_host(gpu, orc):
    # (m) on the circuit whose leaves hold a word below 2^32 - 1: the host takes every word mod p, and so does the table the device reads
    c = _case(gpu, orc, "m2")
    bad = _non_canonical_leaf_word(c.desc, c.proofs[1])
    assert bad is not None and bad != c.proofs[1] and len(bad) == len(c.proofs[1])
    bv = c.cd.batch_verifier(max_batch=2)
    assert bv.verify([c.proofs[0], bad, c.proofs[2]]) == [(True, "")] * 3 and c.cd.verify(bad) == (True, "")


# ------------------------------------------------------------------------------- 3. batch mechanics
def _good_and_bad(c):
    d, by = c.desc, c.proofs[0]
    bad = [b for _, b in _host_stage_mutants(d, by)[:2] + _query_mutants(d, by, c.x_index[0], 9)[:5]]
    return c.proofs, bad


@pytest.mark.gpu
def test_counts_chunks_threads_and_reused_staging(gpu, orc):
    p, ctx = gpu
    c = _case(gpu, orc, "m2")
    good, bad = _good_and_bad(c)
    want = {by: c.cd.verify(by) for by in good + bad}
    assert all(want[by][0] for by in good) and not any(want[by][0] for by in bad)
    one, four = c.cd.batch_verifier(max_batch=4, host_threads=1), c.cd.batch_verifier(max_batch=4, host_threads=4)
    mixed = [good[0], bad[0], bad[1], good[1], bad[2], good[2], bad[3], bad[4], good[0]]       # 2 * max_batch + 1
    for batch in ([], good[:1], bad[:1], [good[0], bad[2], good[1], bad[0]], mixed):
        a, b = one.verify(batch), four.verify(batch)
        assert a == b and one.checks == four.checks and len(a) == len(batch)
        for by, g in zip(batch, a):
            _same(g, want[by])
    # stale flags: after a call full of rejections the same verifier answers as before
    first = one.verify(mixed)
    assert not any(ok for ok, _ in one.verify(bad[:4]))
    assert one.verify(mixed) == first and one.verify(good) == [(True, "")] * len(good)
    # checks = NULL is accepted
    n = len(mixed)
    ptrs, sizes = (ctypes.c_char_p * n)(*mixed), (ctypes.c_size_t * n)(*[len(b) for b in mixed])
    verdicts = np.full(n, -1, dtype=np.int32)
    assert p._lib.lib.gl_batch_verifier_verify(one.handle, ptrs, sizes, n, verdicts.ctypes.data_as(ctypes.c_void_p), None) == 0
    assert [int(v) for v in verdicts] == [0 if ok else p._lib.GL_ERR_VERIFY for ok, _ in first]
    assert p._lib.lib.gl_batch_verifier_verify(one.handle, None, None, 0, None, None) == 0     # count = 0 reads nothing
    # a proof too short for the description's counts is gl_verify's GL_ERR_ARG, there and here
    with pytest.raises(p.Plonky2Mi355xError) as e1:
        c.cd.verify(good[0][:100])
    with pytest.raises(p.Plonky2Mi355xError) as e2:
        one.verify([good[0], good[0][:100]])
    assert e1.value.code == e2.value.code == 1 and one.checks == [0, p._lib.GL_CHECK_DESCRIPTION]


# ------------------------------------------------------------------------------- 4. two verifiers, two contexts, two threads
@pytest.mark.gpu
def test_two_verifiers_on_two_contexts_from_two_threads(gpu, orc):
    p, ctx = gpu
    c = _case(gpu, orc, "chained")
    good, bad = _good_and_bad(c)
    batches = [[good[0], bad[0], bad[3], good[1], bad[5], bad[6]] * 3, [bad[2], good[0], bad[4], bad[1]] * 4]
    cap, dig = c.cd.constants_sigmas_cap, c.cd.circuit_digest
    bvs = [p.BatchVerifier(c.desc, cap, dig, ctx=p.Context(0), max_batch=8, host_threads=2) for _ in batches]
    want = [(bv.verify(b), list(bv.checks)) for bv, b in zip(bvs, batches)]
    for (answers, _), b in zip(want, batches):
        for by, g in zip(b, answers):
            _same(g, c.cd.verify(by))
    got, errors = [None] * len(bvs), []

    def run(k):
        try:
            for _ in range(3):
                got[k] = (bvs[k].verify(batches[k]), list(bvs[k].checks))
        except Exception as e:                           # noqa: BLE001  (reported below)
            errors.append(e)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(len(bvs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == want


# ------------------------------------------------------------------------------- 5. no GPU needed
NEW_SYMBOLS = ("gl_batch_verifier_new", "gl_batch_verifier_verify", "gl_verify_check_message", "gl_batch_verifier_free")


def test_the_four_symbols_are_declared_exported_and_bound():
    from plonky2_demo_amd import _lib
    from test_abi import declared_symbols
    declared = declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    import plonky2_demo_amd as p
    assert p.BatchVerifier is p.api.BatchVerifier and hasattr(p.api._CircuitApi, "batch_verifier")


def test_check_messages_are_the_texts_of_gl_verifys_rejections(orc):
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    from plonky2_demo_amd.api import verify_check_message
    texts = [verify_check_message(c) for c in range(1, 13)]
    assert verify_check_message(0) == "" and all(texts) and len(set(texts)) == 12
    m = 2
    hc, oc = p.MatmulCircuit(m), orc.circuit(m, threads=4)
    a, b = rand_field(40 + m, m * m) % (2**32 - 1), rand_field(41 + m, m * m) % (2**32 - 1)
    by = oc.witness(a, b, filler_seed=0).prove(threads=4).to_bytes()
    assert hc.verify(by, oc.constants_sigmas_cap, oc.digest) == (True, "")
    mutants = dict(_host_stage_mutants(hc.desc, by))
    codes = {"j: truncated": (_lib.GL_CHECK_TRUNCATED,), "k: trailing byte": (_lib.GL_CHECK_LENGTH,), "a: opening word": (_lib.GL_CHECK_VANISHING,),
             "b: proof-of-work witness": (_lib.GL_CHECK_POW,),
             "l: path length off by one": (_lib.GL_CHECK_STEP_PATH_LENGTH, _lib.GL_CHECK_INITIAL_PATH_LENGTH, _lib.GL_CHECK_TRUNCATED)}
    for what, expected in codes.items():
        ok, why = hc.verify(mutants[what], oc.constants_sigmas_cap, oc.digest)
        assert not ok
        assert sum(why.startswith(verify_check_message(c) + " (") for c in expected) == 1, (what, why)
        assert sum(why.startswith(t + " (") for t in texts) == 1, (what, why)


def test_new_refuses_null_arguments_and_an_empty_batch():
    import plonky2_demo_amd as p
    from plonky2_demo_amd._lib import lib
    hc = p.MatmulCircuit(2)
    cap, dig = np.zeros((16, 4), dtype=U64), np.zeros(4, dtype=U64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    not_a_context = ctypes.create_string_buffer(4096)    # the argument checks come before anything reads the context
    h = ctypes.c_void_p()
    assert lib.gl_batch_verifier_new(None, ctypes.byref(hc.desc), vp(cap), vp(dig), 4, 1, ctypes.byref(h)) == 1 and not h.value
    assert lib.gl_batch_verifier_new(ctypes.cast(not_a_context, ctypes.c_void_p), ctypes.byref(hc.desc), vp(cap), vp(dig), 4, 1, None) == 1
    assert lib.gl_batch_verifier_new(ctypes.cast(not_a_context, ctypes.c_void_p), ctypes.byref(hc.desc), vp(cap), vp(dig), 0, 1, ctypes.byref(h)) == 1
    assert b"max_batch" in lib.gl_last_error() and not h.value
    assert lib.gl_batch_verifier_new(ctypes.cast(not_a_context, ctypes.c_void_p), ctypes.byref(hc.desc), vp(cap), vp(dig), 4097, 1, ctypes.byref(h)) == 1
    lib.gl_batch_verifier_free(None)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import plonky2_demo_amd as p
    hc = p.MatmulCircuit(2)
    with pytest.raises(p.Plonky2Mi355xError):
        p.BatchVerifier(hc.desc, np.zeros((16, 4), dtype=U64), np.zeros(4, dtype=U64))
