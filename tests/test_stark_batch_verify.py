"""The batch STARK verifier (gl_stark_batch_verifier: host stage per proof, the FRI query phase of a whole batch on the device) against
gl_stark_verify / gl_stark_dag_verify: for every proof of a call the same verdict and the same first failing check as the single
call gives for that proof alone -- on valid proofs of the AIRs of stark_airs.py and of a DAG AIR, on the three committed proofs with
64 seeded bit flips each, on a tamper matrix laid out from the documented proof layout, across chunks and host threads.  The tests at
the end need no GPU."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import fri_openings_model as fm
import stark_airs
import stark_dag_airs as da
import stark_dag_model as dm
import stark_model as sm
from test_fri_openings import Layout, flip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U64 = np.uint64
GL_ERR_ARG, GL_ERR_UNSUPPORTED = 1, 3


def config_of(p, air, nc=2):
    c = p.StarkConfig.standard_fast_config()
    c.num_challenges, c.rate_bits = nc, air.rate_bits
    return c


def desc_of(p, air):
    if hasattr(air, "dag_constraints"):
        return dm.desc_of(p, air)
    return p.StarkDesc(air.num_columns, air.num_public_inputs, air.constraint_degree, air.constraints, air.pairs)


def same(got, host):
    """the batch's (accepted, message, code) against the single call's: the host's message carries the source position behind it"""
    assert (got[0], got[2]) == (host[0], host[2]), (got, host)
    if host[0]:
        assert got[1] == "" and host[1] == "" and got[2] == 0
    else:
        assert got[1] and host[1].startswith(got[1] + " ("), (got, host)


def check_batch(p, bv, desc, config, lg_n, hasher, proofs):
    """one batch call; every proof held against the single host call -> the batch's answers"""
    got = bv.verify(proofs)
    assert len(got) == len(proofs)
    for g, by in zip(got, proofs):
        same(g, p.stark_verify(desc, config, lg_n, by, hasher=hasher))
    return got


# ------------------------------------------------------------------------------- proofs, made once
_cases = {}


def traces_of(air, n):
    if air.name == "fibonacci":
        return [air.trace(n, 0, k, 2 * k + 1) for k in range(3)]      # (its generator takes the first two numbers, not a seed)
    return [air.trace(n, seed=k) for k in range(3)]


def stark_case(gpu, name, lg_n, nc=2, hasher="poseidon"):
    """the Stark on the device with proofs of three different traces: zeta, the points and the caps differ per proof"""
    key = (name, lg_n, nc, hasher)
    if key not in _cases:
        p, ctx = gpu
        air = da.EVERY[name] if name in da.OWN else stark_airs.AIRS[name]
        desc, config = desc_of(p, air), config_of(p, air, nc)
        stark = p.Stark(desc, config, lg_n, hasher=hasher, ctx=ctx)
        proofs = [stark.prove(trace, pis) for trace, pis in traces_of(air, 1 << lg_n)]
        assert len(set(proofs)) == 3
        _cases[key] = SimpleNamespace(air=air, desc=desc, config=config, lg_n=lg_n, nc=nc, hasher=hasher, stark=stark, proofs=proofs, params=stark.params)
    return _cases[key]


VALID = [("fibonacci", 5, 2, "poseidon"), ("fibonacci", 7, 2, "poseidon"), ("fibonacci", 11, 2, "poseidon"), ("fibonacci", 7, 2, "keccak"),
         ("nopublic", 5, 2, "poseidon"), ("wide", 5, 2, "poseidon"), ("nonic", 5, 4, "poseidon"), ("quartic", 7, 3, "poseidon"),
         ("longpair", 5, 3, "poseidon"), ("sbox2", 5, 2, "poseidon")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lg_n,nc,hasher", VALID, ids=["%s-%d-%d-%s" % v for v in VALID])
def test_valid_proofs_are_accepted_as_by_the_host(gpu, name, lg_n, nc, hasher):
    p, ctx = gpu
    c = stark_case(gpu, name, lg_n, nc, hasher)
    assert len(c.params.reduction_arity_bits) == {5: 0, 7: 1, 11: 2}[lg_n]
    if name == "nonic":
        assert (c.air.q, c.params.rate_bits) == (8, 3)
    if name == "wide":
        assert c.air.num_columns == 130 and not c.air.pairs
    bv = c.stark.batch_verifier()
    got = check_batch(p, bv, c.desc, c.config, lg_n, hasher, c.proofs)
    assert got == [(True, "", 0)] * 3
    if name == "sbox2":
        assert all(p.stark_dag_verify(c.desc, c.config, lg_n, by) == (True, "", 0) for by in c.proofs)


# ------------------------------------------------------------------------------- the three committed proofs, 64 bit flips each
def load_fixture(p, stem):
    with open(os.path.join(GOLDEN, stem + ".bin"), "rb") as f:
        proof = f.read()
    with open(os.path.join(GOLDEN, stem + ".json")) as f:
        meta = json.load(f)
    air = da.EVERY[meta["air"]] if meta["air"] in da.OWN else stark_airs.AIRS[meta["air"]]
    config = config_of(p, air, meta["num_challenges"])
    lg_n = meta["params"]["degree_bits"]
    params = config.fri_params(lg_n)
    assert {k: getattr(params, k) for k in meta["params"]} == meta["params"] and meta["num_bytes"] == len(proof)
    return proof, desc_of(p, air), config, lg_n


@pytest.mark.gpu
@pytest.mark.parametrize("stem", ["stark_fibonacci_n32", "stark_nonic_n32_nc3", "stark_dag_sbox2_n32"])
def test_a_committed_proof_and_64_bit_flips_get_the_hosts_verdicts(gpu, stem):
    p, ctx = gpu
    proof, desc, config, lg_n = load_fixture(p, stem)
    rng = np.random.default_rng(2027)
    proofs = [proof]
    for k in range(64):                                   # spread over the whole byte range: one flip per 64th of the proof
        lo, hi = len(proof) * k // 64, len(proof) * (k + 1) // 64
        proofs.append(flip(proof, int(rng.integers(lo, hi)), int(rng.integers(0, 8))))
    bv = p.StarkBatchVerifier(desc, config, lg_n, ctx=ctx, max_batch=65, host_threads=2)
    got = check_batch(p, bv, desc, config, lg_n, "poseidon", proofs)       # equality with the host, whatever the host says; no flip excluded
    assert got[0] == (True, "", 0)
    assert len({code for _, _, code in got}) >= 3         # (accepted, and rejections of both stages)


# ------------------------------------------------------------------------------- a tamper matrix from the documented layout
class StarkLayout:
    """byte offsets inside a STARK proof (include/plonky2_mi355x.h): caps, the five opening groups, the FriProof, the public inputs"""

    def __init__(self, air, nc, params):
        hb = 25 if params.hasher else 32
        nz, nq = sm.num_zs(air, nc), air.q * nc
        oracles = [air.num_columns] + ([nz] if nz else []) + [nq]
        self.caps, at = [], 0
        for _ in oracles:
            self.caps.append(at)
            at += hb << params.cap_height
        self.openings = {}
        for group, k in (("local", air.num_columns), ("next", air.num_columns), ("zs", nz), ("zs_next", nz), ("quotient", nq)):
            self.openings[group] = at
            at += 16 * k
        self.fri = at
        self.lay = Layout(params, SimpleNamespace(oracles=[(k, False) for k in oracles]))
        self.public_inputs = at + self.lay.size
        self.size = self.public_inputs + 8 * air.num_public_inputs


@pytest.mark.gpu
@pytest.mark.parametrize("lg_n", [7, 11])
def test_a_tamper_matrix_on_fibonacci_gets_the_hosts_verdict_and_first_failing_check(gpu, lg_n):
    p, ctx = gpu
    c = stark_case(gpu, "fibonacci", lg_n)
    by = c.proofs[1]
    sl = StarkLayout(c.air, c.nc, c.params)
    lay, fri = sl.lay, sl.fri
    assert sl.size == len(by) and len(lay.leaf) == 3
    host = lambda proof: p.stark_verify(c.desc, c.config, lg_n, proof)      # noqa: E731
    # x & 15 of query 0: the one of the sixteen step evals whose change fails the consistency comparison
    codes = [host(flip(by, fri + lay.step_evals[0] + 16 * k))[2] for k in range(16)]
    assert sorted(codes) == [fm.FRI_CONSISTENCY] + [fm.STEP_MERKLE] * 15
    within = codes.index(fm.FRI_CONSISTENCY)
    mutants = [("cap %d" % o, flip(by, at + 9)) for o, at in enumerate(sl.caps)]
    mutants += [("opening in %s" % g, flip(by, at + 8, 5)) for g, at in sl.openings.items()]
    mutants += [("public input", flip(by, sl.public_inputs + 8)), ("commit cap", flip(by, fri + lay.commit_caps + 40, 1))]
    for o in range(3):
        mutants += [("leaf word of oracle %d" % o, flip(by, fri + lay.leaf[o], 3)), ("sibling of oracle %d" % o, flip(by, fri + lay.sibling[o] + 32 + 8, 3))]
    mutants += [("step eval at x & 15", flip(by, fri + lay.step_evals[0] + 16 * within, 3)),
                ("another step eval", flip(by, fri + lay.step_evals[0] + 16 * ((within + 5) & 15) + 8, 3))]
    if lg_n == 11:                                        # (at 2^7 the step paths are empty under the cap)
        mutants.append(("step sibling", flip(by, fri + lay.step_sibling[0] + 32 + 16, 3)))
    mutants += [("final coefficient", flip(by, fri + lay.final + 24, 1)), ("PoW witness", flip(by, fri + lay.pow, 1)),
                ("truncated by one byte", by[:-1]), ("one trailing byte", by + b"\0")]
    proofs = []
    for k, (_, bad) in enumerate(mutants):                # one call, the mutants between valid proofs
        proofs += [c.proofs[k % 3], bad]
    got = check_batch(p, c.stark.batch_verifier(max_batch=64, host_threads=2), c.desc, c.config, lg_n, "poseidon", proofs)
    answers = {name: got[2 * k + 1] for k, (name, _) in enumerate(mutants)}
    assert all(got[2 * k] == (True, "", 0) for k in range(len(mutants))) and not any(ok for ok, _, _ in answers.values())
    assert answers["leaf word of oracle 1"][2] == answers["sibling of oracle 2"][2] == fm.INITIAL_MERKLE
    assert answers["step eval at x & 15"][2] == fm.FRI_CONSISTENCY and answers["another step eval"][2] == fm.STEP_MERKLE
    assert answers["public input"][2] == answers["opening in quotient"][2] == fm.VANISHING
    assert answers["truncated by one byte"][2] == fm.TRUNCATED and answers["one trailing byte"][2] == fm.LENGTH
    if lg_n == 11:
        assert answers["step sibling"][2] == fm.STEP_MERKLE


# ------------------------------------------------------------------------------- chunks and threads
@pytest.mark.gpu
def test_chunks_threads_and_reused_staging(gpu):
    p, ctx = gpu
    c = stark_case(gpu, "fibonacci", 7)
    sl = StarkLayout(c.air, c.nc, c.params)
    good = c.proofs
    bad = [flip(good[0], sl.fri + sl.lay.leaf[0]), flip(good[1], sl.openings["next"] + 3), flip(good[2], sl.fri + sl.lay.step_evals[0] + 83 * sl.lay.query_len),
           good[0][:-1], flip(good[1], sl.fri + sl.lay.sibling[2] + 5 + 40 * sl.lay.query_len)]
    nine = [good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], good[0], bad[4]]       # 2 * max_batch + 1, bad proofs on both sides of a boundary
    one, four = c.stark.batch_verifier(max_batch=4, host_threads=1), c.stark.batch_verifier(max_batch=4, host_threads=4)
    a = check_batch(p, four, c.desc, c.config, 7, "poseidon", nine)
    assert a == one.verify(nine) and [ok for ok, _, _ in a] == [True, False, True, False, False, True, False, True, False]
    assert four.verify([]) == [] and four.verify(good[:1]) == [(True, "", 0)]
    # stale flags: after a batch full of rejections the same verifier accepts a good batch
    assert not any(ok for ok, _, _ in four.verify(bad[:4]))
    assert four.verify(good + good[:1]) == [(True, "", 0)] * 4


# ------------------------------------------------------------------------------- no GPU needed
NEW_SYMBOLS = ("gl_stark_batch_verifier_new", "gl_stark_batch_verifier_verify", "gl_stark_batch_verifier_free")


def test_the_symbols_are_declared_exported_and_bound():
    import plonky2_demo_amd as p
    from plonky2_demo_amd import _lib
    from test_abi import declared_symbols
    declared = declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert p.StarkBatchVerifier is p.api.StarkBatchVerifier and hasattr(p.api.Stark, "batch_verifier")


def test_new_refuses_null_arguments_limits_hiding_and_other_arities():
    import plonky2_demo_amd as p
    from plonky2_demo_amd._lib import lib
    air = stark_airs.fibonacci
    desc, config = desc_of(p, air).struct(2), config_of(p, air)
    params = config.fri_params(7)
    not_a_context = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)      # the argument checks come before anything reads the context
    h = ctypes.c_void_p()
    new = lib.gl_stark_batch_verifier_new
    assert new(None, ctypes.byref(desc), None, ctypes.byref(params), 4, 1, ctypes.byref(h)) == GL_ERR_ARG and not h.value
    assert new(not_a_context, None, None, ctypes.byref(params), 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    assert new(not_a_context, ctypes.byref(desc), None, None, 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    assert new(not_a_context, ctypes.byref(desc), None, ctypes.byref(params), 4, 1, None) == GL_ERR_ARG
    for max_batch in (0, 4097):
        assert new(not_a_context, ctypes.byref(desc), None, ctypes.byref(params), max_batch, 1, ctypes.byref(h)) == GL_ERR_ARG
        assert b"max_batch" in lib.gl_last_error() and not h.value
    assert new(not_a_context, ctypes.byref(desc), None, ctypes.byref(params), 4, 65, ctypes.byref(h)) == GL_ERR_ARG
    # gl_stark_check's refusals, with its codes
    hiding = config.fri_params(7)
    hiding.hiding = 1
    for bad in (hiding, p.FriParams(7, 1, 4, 16, 84, [3]), p.FriParams(7, 1, 4, 16, 84, [9])):
        want = lib.gl_stark_check(ctypes.byref(desc), ctypes.byref(bad))
        text = lib.gl_last_error()
        assert want in (GL_ERR_ARG, GL_ERR_UNSUPPORTED)
        assert new(not_a_context, ctypes.byref(desc), None, ctypes.byref(bad), 4, 1, ctypes.byref(h)) == want and not h.value
        assert lib.gl_last_error().split(b" (")[0] == text.split(b" (")[0]
    assert lib.gl_stark_check(ctypes.byref(desc), ctypes.byref(hiding)) == GL_ERR_UNSUPPORTED
    assert lib.gl_stark_check(ctypes.byref(desc), ctypes.byref(p.FriParams(7, 1, 4, 16, 84, [3]))) == GL_ERR_UNSUPPORTED
    # a term list beside a dag is gl_stark_dag_check's refusal
    dag = dm.desc_of(p, da.EVERY["sbox2"])
    assert new(not_a_context, ctypes.byref(desc), ctypes.byref(dag.dag_struct()), ctypes.byref(params), 4, 1, ctypes.byref(h)) == GL_ERR_ARG
    lib.gl_stark_batch_verifier_free(None)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import plonky2_demo_amd as p
    with pytest.raises(p.Plonky2Mi355xError):
        p.StarkBatchVerifier(desc_of(p, stark_airs.fibonacci), config_of(p, stark_airs.fibonacci), 7)
