"""FRI openings of any instance: gl_fri_combine_instance, gl_prove_openings, gl_verify_openings (PolynomialBatch::prove_openings,
fri/oracle.rs:162-219; verify_fri_proof, fri/verifier.rs:62-241) against the Python-integer model of fri_openings_model.py.

  A  combine and divide by value (k_fri_combine_points, k_div_points_*) at every size where the kernels take another path
  B  the Plonk instance through the generic path: byte for byte what gl_fri_combine gives, and the FRI section of gl_prove's proof
  C  a STARK-shaped instance (rate_bits 1, 84 queries, 16 bits of work) end to end, library verifier and model verifier
  D  the phase form assembled by a caller equals the one-call form
  E  the tamper matrix: one flipped word per case, the check named
  F  (CPU) the committed GPU-made proof: both verifiers accept it and reject the same 64 bit flips
  G  (CPU) the validation table, and a hand-assembled proof with a reduction of arity 8
"""
import ctypes
import json
import os

import numpy as np
import pytest

import fri_openings_model as fm
import prover_phase_model as pm
from oracle_lib import P, rand_field
from transcript import LibraryChallenger, drive_phase_api, poseidon_challenger
from vanishing_model import primitive_root

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U64 = np.uint64
M64 = (1 << 64) - 1
GL_ERR_ARG, GL_ERR_UNSUPPORTED, GL_ERR_VERIFY = 1, 3, 6
NO_PIS = np.zeros(0, dtype=U64)


# ------------------------------------------------------------------------------- shared helpers
def columns_of(seed, ncols, n):
    """[ncols][n] coefficients with 0, 1 and p - 1 among them (first column, last column, last coefficient)"""
    c = rand_field(seed, (ncols, n))
    c[0, :3] = [0, 1, P - 1]
    c[-1, -1] = P - 1
    c[-1, 0] = 0
    return c


def build_oracles(p, ctx, widths, blinding, lg_n, rate_bits, cap_height, seed, hasher="poseidon"):
    cols = [columns_of(1000 * seed + o, w, 1 << lg_n) for o, w in enumerate(widths)]
    batches = [p.PolynomialBatch.from_coeffs_blinded(c, rate_bits, cap_height, seed=bytes([o + 1] * 32), ctx=ctx, hasher=hasher) if b
               else p.PolynomialBatch.from_coeffs(c, rate_bits, False, cap_height, ctx=ctx, hasher=hasher) for o, (c, b) in enumerate(zip(cols, blinding))]
    return cols, batches


def ext_tuples(a):
    return [(int(x), int(y)) for x, y in np.asarray(a, dtype=U64).reshape(-1, 2)]


def scaled(point, g):
    return (int(point[0]) % P * g % P, int(point[1]) % P * g % P)


def model_challenger(orc, hasher):
    if hasher == "keccak":
        import test_keccak
        return test_keccak.model_challenger()
    return poseidon_challenger(orc)


def verify_path_of(orc, hasher):
    if hasher == "keccak":
        import test_keccak
        return lambda leaf, index, cap, siblings: bool(test_keccak.model_verify_path(leaf, index, np.array(siblings, dtype=U64).reshape(-1, 4), cap))
    return fm.poseidon_verify_path(orc)


def absorb(ch, caps, openings):
    """what a caller's transcript holds before prove_openings: here the oracle caps and the openings"""
    for cap in caps:
        ch.observe_hashes(cap)
    ch.observe(np.asarray(openings, dtype=U64).reshape(-1))
    return ch


def library_challenger(p, hasher, caps, openings):
    return absorb(LibraryChallenger(p, hasher), caps, openings).ch


class Layout:
    """byte offsets inside a FriProof (write_fri_proof order)"""

    def __init__(self, params, instance):
        hb = 25 if params.hasher else 32
        arity = params.reduction_arity_bits
        lgN, ncap = params.degree_bits + params.rate_bits, 1 << params.cap_height
        self.commit_caps = 0
        at = len(arity) * ncap * hb
        self.query0 = at
        self.leaf, self.sibling, self.leaf_len = [], [], []
        for k, blinding in instance.oracles:
            k += 4 if params.hiding and blinding else 0
            self.leaf.append(at)
            self.leaf_len.append(k)
            self.sibling.append(at + 8 * k + 1)
            at += 8 * k + 1 + (lgN - params.cap_height) * hb
        self.step_evals, self.step_sibling, lg = [], [], lgN
        for ab in arity:
            lg -= ab
            self.step_evals.append(at)
            self.step_sibling.append(at + 8 * (2 << ab) + 1)
            at += 8 * (2 << ab) + 1 + (lg - params.cap_height) * hb
        self.query_len = at - self.query0
        self.final = self.query0 + params.num_query_rounds * self.query_len
        self.pow = self.final + 16 * ((1 << params.degree_bits) >> sum(arity))
        self.size = self.pow + 8


def flip(by, offset, bit=0):
    b = bytearray(by)
    b[offset] ^= 1 << bit
    return bytes(b)


# ------------------------------------------------------------------------------- A: combine and divide by value
ALPHAS = {"random": None, "zero": (0, 0), "one": (1, 0), "noncanonical": (P + 2, M64)}
POINTS = {"random": (0, 0), "zero": (1, 0), "one": (P - 1, P - 1), "noncanonical": (P + 5, M64 - 2)}      # the point that goes with each alpha
_oracle_cache = {}


def instance_a(p, which, lg_n, point):
    g = primitive_root(lg_n)
    if which == "one":
        return [1], [False], False, p.FriInstance([(1, False)], [(point, [(0, 0)])])
    if which == "three":
        widths, blinding = [5, 3, 2], [False, True, False]
        everything = [(o, c) for o, w in enumerate(widths) for c in range(w)]
        second = [(0, c) for c in range(5)] + [(1, 0), (0, 2)]                 # oracle 0 plus (1, 0), with (0, 2) listed twice
        batches = [(point, everything), (scaled(point, g), second), ((3, 0), [(2, 1)])]
        return widths, blinding, True, p.FriInstance(list(zip(widths, blinding)), batches)
    widths = [200, 61]                                                          # 261 columns: more than 256, no multiple of 4
    return widths, [False, False], False, p.FriInstance([(w, False) for w in widths], [(point, [(o, c) for o, w in enumerate(widths) for c in range(w)])])


def run_combine(gpu, which, lg_n, alpha_name):
    p, ctx = gpu
    alpha = ALPHAS[alpha_name] or tuple(int(x) for x in rand_field(77 + lg_n, 2))
    widths, blinding, hiding, inst = instance_a(p, which, lg_n, POINTS[alpha_name])
    key = (which, lg_n)
    if key not in _oracle_cache:
        _oracle_cache[key] = build_oracles(p, ctx, widths, blinding, lg_n, 1, 2, seed=lg_n)
    cols, batches = _oracle_cache[key]
    params = p.FriParams(lg_n, 1, 2, 0, 1, [], hiding=hiding)                   # no reduction: the final polynomial is all n coefficients
    fri = p.FriProver.from_instance(inst, batches, alpha, params, ctx=ctx)
    got = ext_tuples(fri.final_poly())
    want = fm.final_poly(inst, cols, alpha)
    bad = [k for k in range(1 << lg_n) if got[k] != want[k]]
    assert not bad, "%d coefficients differ, first %d: got %s, want %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("alpha_name", list(ALPHAS))
@pytest.mark.parametrize("lg_n", [4, 6, 11])
@pytest.mark.parametrize("which", ["one", "three", "wide"])
def test_combine_and_divide_equal_the_model(gpu, which, lg_n, alpha_name):
    # n = 16: under one workgroup's 64 coefficients and one 32-coefficient segment; 64: two segments; 2^11: 64 segments, the carries scan
    # spans several waves
    run_combine(gpu, which, lg_n, alpha_name)


@pytest.mark.gpu
def test_combine_and_divide_over_1024_segments_of_64(gpu):
    run_combine(gpu, "three", 16, "random")


@pytest.mark.gpu
@pytest.mark.parametrize("which,lg_n", [("three", 4), ("three", 11), ("wide", 6)])
def test_one_pass_equals_the_per_batch_sequence(gpu, which, lg_n):
    # the diagnostic entry point runs gl_fri_combine's kernels, one batch after the other: the same coefficients
    p, ctx = gpu
    widths, blinding, hiding, inst = instance_a(p, which, lg_n, POINTS["noncanonical"])
    if (which, lg_n) not in _oracle_cache:
        _oracle_cache[(which, lg_n)] = build_oracles(p, ctx, widths, blinding, lg_n, 1, 2, seed=lg_n)
    batches = _oracle_cache[(which, lg_n)][1]
    params = p.FriParams(lg_n, 1, 2, 0, 1, [], hiding=hiding)
    one_pass, per_batch = (p.FriProver.from_instance(inst, batches, (11, 12), params, ctx=ctx, per_batch=pb).final_poly() for pb in (False, True))
    assert (one_pass == per_batch).all()


# ------------------------------------------------------------------------------- B: the Plonk instance, byte for byte
class Recorder:
    """a challenger that remembers what it handed out"""

    def __init__(self, ch):
        self.ch, self.gets = ch, []

    def observe(self, xs):
        self.ch.observe(xs)

    def observe_hashes(self, digests, inner=False):
        self.ch.observe_hashes(digests, inner=inner)

    def get(self, k):
        self.gets.append(self.ch.get(k))
        return self.gets[-1]

    @property
    def state(self):
        return self.ch.state

    @property
    def inp(self):
        return self.ch.inp


def plonk_instance(p, d, zeta, gzeta):
    """the four oracles and two batches of glfri::PlonkInstance (fri_instance.hpp), in prover_phase_model.opened_polys order"""
    ncs, nzs = d.num_constants + 80, 20 + 2 * d.num_lookup_polys
    names = [[(o, c) for c in range(w)] for o, w in enumerate((ncs, 135, nzs, 16))]
    at_zeta, at_gzeta = pm.opened_polys(names)
    return p.FriInstance([(ncs, False), (135, False), (nzs, False), (16, False)], [(zeta, at_zeta), (gzeta, at_gzeta)])


def check_plonk_route(gpu, orc, cd, wires, pis, hasher, rounds):
    p, ctx = gpu
    d = cd.desc
    assert d.num_fri_rounds == rounds
    rec = Recorder(LibraryChallenger(p, hasher))
    r = drive_phase_api(p, ctx, orc, cd, rec, wires, pis)
    betas = rec.gets[len(rec.gets) - d.num_query_rounds - 1 - rounds:len(rec.gets) - d.num_query_rounds - 1]
    inst = plonk_instance(p, d, r.zeta, r.gzeta)
    assert inst.num_opened == sum(len(np.asarray(v).reshape(-1, 2)) for v in r.openings.values())
    fri = p.FriProver.from_instance(inst, r.batches, r.fri_alpha, p.FriParams.of_circuit(d), ctx=ctx)
    for k in range(rounds):
        assert (fri.commit_round() == r.fri_caps[k]).all(), "commit cap %d" % k
        fri.fold(betas[k])
    assert (fri.final_poly() == r.final_poly).all()
    assert fri.query(r.x_index) == r.query_blob


def _plonk_circuits(p, ctx, orc, which):
    """(circuit data, wires, public inputs, hasher, reduction rounds): the circuits of the two tests above"""
    if which == "lookups":
        oc = orc.circuit_of_kind(8, 50, threads=8)
        w = oc.witness(np.arange(3, 53, dtype=U64), NO_PIS, filler_seed=9)
        cd = p.GenericCircuitData(oc.product_desc(), oc.constants_sigmas())
        assert cd.desc.num_lookup_polys
        return cd, w.wires(), w.public_inputs(), "poseidon", cd.desc.num_fri_rounds
    import ext_gate_circuits as egc
    lg_n, hasher, rounds = which
    c = egc.Chained(seed=3, min_degree_bits=lg_n, hasher=1 if hasher == "keccak" else 0).circuit
    return p.GenericCircuitData.from_classes(c.desc, c.constants, c.classes, ctx=ctx), c.wires(), NO_PIS, hasher, rounds


@pytest.mark.gpu
@pytest.mark.parametrize("lg_n,hasher,rounds", [(6, "poseidon", 1), (6, "keccak", 1), (10, "poseidon", 2)])
def test_plonk_instance_reproduces_the_plonk_path(gpu, orc, lg_n, hasher, rounds):
    check_plonk_route(gpu, orc, *_plonk_circuits(gpu[0], gpu[1], orc, (lg_n, hasher, rounds)))


@pytest.mark.gpu
def test_plonk_instance_with_lookups_reproduces_the_plonk_path(gpu, orc):
    check_plonk_route(gpu, orc, *_plonk_circuits(gpu[0], gpu[1], orc, "lookups"))


@pytest.mark.gpu
@pytest.mark.parametrize("which", [(6, "poseidon", 1), (6, "keccak", 1), (10, "poseidon", 2), "lookups"], ids=str)
def test_prove_openings_on_the_plonk_instance_writes_the_fri_section_of_the_circuit_proof(gpu, orc, which):
    """A circuit proof is one more FRI instance on the prover side (the mirror of the cut-out test below): gl_prove_openings on
    plonk_instance, over the four batches of the phase API and a Challenger advanced through the Plonk transcript up to the observed
    openings, writes the bytes that stand in gl_prove's proof between the OpeningSet and the public inputs."""
    from proof_parser import ParsedProof, hash_bytes, opening_columns
    from transcript import replay_to_openings
    p, ctx = gpu
    cd, wires, pis, hasher, rounds = _plonk_circuits(p, ctx, orc, which)
    d = cd.desc
    assert d.num_fri_rounds == rounds
    r = drive_phase_api(p, ctx, orc, cd, LibraryChallenger(p, hasher), wires, pis)
    by = cd.prove(wires, pis).to_bytes()
    pp = ParsedProof(d, by)
    fri_at = (3 << d.cap_height) * hash_bytes(d) + 16 * sum(k for _, k in opening_columns(d))
    fri_end = len(by) - 8 * (1 + len(pp.public_inputs))                          # behind the proof-of-work witness
    ch = LibraryChallenger(p, hasher)
    zeta = replay_to_openings(d, ch, cd.circuit_digest, r.pi_hash, pp)[-1]
    assert list(zeta) == list(r.zeta)
    inst = plonk_instance(p, d, r.zeta, r.gzeta)
    got = p.PolynomialBatch.prove_openings(inst, r.batches, ch.ch, p.FriParams.of_circuit(d), ctx=ctx)
    assert len(got) == fri_end - fri_at and got == by[fri_at:fri_end]


# ------------------------------------------------------------------------------- B': the verifier side of the same fact (CPU)
def _circuit_proofs(p, orc, name):
    """(description, constants_sigmas_cap, circuit digest, proof bytes): oracle-made matmul proofs, or the committed GPU-made one"""
    if name == "ext_gates":
        import ext_gate_circuits as egc
        d = egc.isolated([egc.ARITHMETIC_EXT, egc.MUL_EXT, egc.REDUCING, egc.REDUCING_EXT], 77, rows_per_gate=1).desc
        with open(os.path.join(GOLDEN, "ext_gates_n8_proof.bin"), "rb") as f:
            by = f.read()
        with open(os.path.join(GOLDEN, "ext_gates_n8_verifier_only.bin"), "rb") as f:
            cap, digest, _ = p.api.verifier_only_from_bytes(f.read())
        return d, cap, digest, by
    m = {"m2": 2, "m8": 8}[name]
    oc = orc.circuit(m, threads=8)
    a, b = rand_field(40 + m, m * m) % (2**32 - 1), rand_field(41 + m, m * m) % (2**32 - 1)
    return p.MatmulCircuit(m).desc, oc.constants_sigmas_cap, oc.digest, oc.witness(a, b, filler_seed=0).prove(threads=8).to_bytes()


@pytest.mark.parametrize("name,rounds", [("m2", 0), ("m8", 1), ("ext_gates", 0)])
def test_the_fri_proof_cut_out_of_a_circuit_proof_gets_gl_verifys_check_from_gl_verify_openings(orc, name, rounds):
    """A circuit proof is one more FRI instance, on the verifier side too: the FriProof section of its bytes, with plonk_instance, the
    four caps, the openings in batch order and a Challenger advanced through the Plonk transcript up to the observed openings, is
    accepted by gl_verify_openings where gl_verify accepts the whole proof, and for every mutant of test_batch_verify.py's query matrix
    ((d) - (h) at queries 0 and 27) and the path-length mutant (l) both give the same GL_CHECK_* code."""
    import plonky2_demo_amd as p
    from proof_parser import ParsedProof, hash_bytes, opening_columns
    from proof_mutants import _host_stage_mutants, _query_mutants
    from transcript import FRI_OPENINGS, public_inputs_hash, replay_to_openings, replay_transcript
    d, cap, digest, by = _circuit_proofs(p, orc, name)
    assert d.num_fri_rounds == rounds and d.num_query_rounds == 28
    pp = ParsedProof(d, by)
    pi_hash = public_inputs_hash(orc, pp.public_inputs)
    g = primitive_root(d.degree_bits)
    fri_at = (3 << d.cap_height) * hash_bytes(d) + 16 * sum(k for _, k in opening_columns(d))
    fri_end = len(by) - 8 * (1 + len(pp.public_inputs))                          # behind the proof-of-work witness
    texts = {p.api.verify_check_message(c): c for c in range(1, 15)}

    def whole(proof):
        b = np.frombuffer(proof, dtype=np.uint8)
        ok, why = p.api._verdict(p.api.lib.gl_verify(ctypes.byref(d), p.api._p(p.api._u64(cap)), p.api._p(p.api._u64(digest)), p.api._p(b), b.size))
        return 0 if ok else texts[why.rsplit(" (", 1)[0]]

    def cut_out(proof):
        ch = LibraryChallenger(p, "keccak" if d.hasher else "poseidon")
        zeta = replay_to_openings(d, ch, digest, pi_hash, pp)[-1]                 # (no mutant touches a cap, an opening or a public input)
        inst = plonk_instance(p, d, zeta, scaled(zeta, g))
        caps = np.concatenate([np.asarray(cap, dtype=U64).reshape(1, -1, 4)] + [c.reshape(1, -1, 4) for c in pp.caps])
        openings = np.concatenate([pp.openings[k] for k in FRI_OPENINGS])
        assert inst.num_opened == len(openings) // 2
        return p.verify_fri_proof(inst, caps, openings, ch.ch, proof[fri_at:fri_end], p.FriParams.of_circuit(d))[2]

    assert whole(by) == cut_out(by) == 0
    x_index = replay_transcript(d, LibraryChallenger(p, "keccak" if d.hasher else "poseidon"), digest, pi_hash, pp)[2]
    mutants = [mu for q in (0, 27) for mu in _query_mutants(d, by, x_index, q)] + [mu for mu in _host_stage_mutants(d, by) if mu[0].startswith("l:")]
    assert len(mutants) == 2 * (6 + 3 * rounds) + 1
    seen = set()
    for what, bad in mutants:
        assert len(bad) == len(by)
        code = whole(bad)
        assert code == cut_out(bad) != 0, what
        seen.add(code)
    assert len(seen) >= (4 if rounds else 2)                                      # path length, initial Merkle; consistency and step Merkle


# ------------------------------------------------------------------------------- C: a STARK-shaped instance end to end
STARK_WIDTHS = [7, 2, 4]            # trace, permutation Z, quotient chunks (starky/src/prover.rs)


def stark_arity(lg_n, rate_bits, cap_height):
    """ConstantArityBits(4, 5) (fri/reduction_strategies.rs:39-49)"""
    out = []
    while lg_n > 5 and lg_n + rate_bits - 4 >= cap_height:
        out.append(4)
        lg_n -= 4
    return out


def stark_instance(p, lg_n, zeta, blinding=(False, False, False)):
    g = primitive_root(lg_n)
    everything = [(o, c) for o, w in enumerate(STARK_WIDTHS) for c in range(w)]
    return p.FriInstance(list(zip(STARK_WIDTHS, blinding)), [(zeta, everything), (scaled(zeta, g), [oc for oc in everything if oc[0] < 2])])


class StarkCase:
    """oracles, openings and the proof of one STARK-shaped instance, made once and left unchanged"""

    def __init__(self, gpu, lg_n, hasher, num_queries=84, blinding=(False, False, False)):
        p, ctx = gpu
        self.hasher, self.lg_n = hasher, lg_n
        self.params = p.FriParams(lg_n, 1, 4, 16, num_queries, stark_arity(lg_n, 1, 4), hiding=any(blinding), hasher=hasher)
        zeta = tuple(int(x) for x in rand_field(900 + lg_n, 2))
        self.instance = stark_instance(p, lg_n, zeta, blinding)
        self.cols, self.batches = build_oracles(p, ctx, STARK_WIDTHS, blinding, lg_n, 1, 4, seed=50 + lg_n, hasher=hasher)
        self.caps = np.array([b.cap for b in self.batches], dtype=U64)
        gzeta = self.instance.batches[1][0]
        self.openings = np.concatenate([b.open_at(zeta) for b in self.batches] + [b.open_at(gzeta) for b in self.batches[:2]])
        self.proof = p.PolynomialBatch.prove_openings(self.instance, self.batches, self.challenger(p), self.params, ctx=ctx)

    def challenger(self, p):
        return library_challenger(p, self.hasher, self.caps, self.openings)

    def model(self, orc, proof=None, caps=None, openings=None, max_queries=None, trace=None):
        caps, openings = self.caps if caps is None else caps, self.openings if openings is None else openings
        ch = absorb(model_challenger(orc, self.hasher), caps, openings)
        return fm.verify(self.params, self.instance, caps, openings, ch, self.proof if proof is None else proof, verify_path_of(orc, self.hasher),
                         max_queries=max_queries, trace=trace)

    def library(self, p, proof=None, caps=None, openings=None):
        caps, openings = self.caps if caps is None else caps, self.openings if openings is None else openings
        return p.verify_fri_proof(self.instance, caps, openings, library_challenger(p, self.hasher, caps, openings), self.proof if proof is None else proof,
                                  self.params)


_stark_cache = {}


def stark_case(gpu, lg_n, hasher="poseidon", **kw):
    key = (lg_n, hasher, tuple(sorted(kw.items())))
    if key not in _stark_cache:
        _stark_cache[key] = StarkCase(gpu, lg_n, hasher, **kw)
    return _stark_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("lg_n,hasher,model_queries", [(7, "poseidon", None), (11, "poseidon", 8), (7, "keccak", None)])
def test_stark_shaped_openings_end_to_end(gpu, orc, lg_n, hasher, model_queries):
    p, ctx = gpu
    case = stark_case(gpu, lg_n, hasher)
    assert len(case.params.reduction_arity_bits) == (1 if lg_n == 7 else 2)
    assert len(case.proof) == Layout(case.params, case.instance).size
    assert ext_tuples(case.openings) == fm.openings_of(case.instance, case.cols)
    assert case.library(p) == (True, "", 0)
    trace = {}
    assert case.model(orc, max_queries=model_queries, trace=trace) == fm.ACCEPTED
    # the final polynomial inside the proof: the model's combine, then one fold per reduction
    coeffs = fm.final_poly(case.instance, case.cols, trace["alpha"])
    for ab, beta in zip(case.params.reduction_arity_bits, trace["betas"]):
        coeffs = pm.fold(coeffs, 1 << ab, beta)
    assert [c for pair in coeffs for c in pair] == trace["proof"].final_poly
    assert trace["pow_response"] >> (64 - 16) == 0


@pytest.mark.gpu
def test_salted_oracle_end_to_end(gpu, orc):
    # hiding: the permutation oracle's leaves end in four salt words, which the Merkle paths cover and fri_combine_initial leaves out
    p, ctx = gpu
    case = stark_case(gpu, 7, num_queries=6, blinding=(False, True, False))
    lay = Layout(case.params, case.instance)
    assert lay.leaf_len == [7, 6, 4] and len(case.proof) == lay.size
    assert case.library(p) == (True, "", 0) and case.model(orc) == fm.ACCEPTED
    salt_word = lay.leaf[1] + 8 * 3                                              # the second salt word of query 0
    bad = flip(case.proof, salt_word)
    assert case.library(p, proof=bad)[0::2] == (False, fm.INITIAL_MERKLE) and case.model(orc, proof=bad) == fm.INITIAL_MERKLE


# ------------------------------------------------------------------------------- D: phase form = one-call form
@pytest.mark.gpu
def test_phase_form_equals_the_one_call_form(gpu):
    p, ctx = gpu
    case = stark_case(gpu, 7)
    ch = case.challenger(p)
    fri = p.FriProver.from_instance(case.instance, case.batches, ch.get_n_challenges(2), case.params, ctx=ctx)
    out = b""
    for _ in case.params.reduction_arity_bits:
        cap = fri.commit_round()
        out += np.ascontiguousarray(cap, dtype="<u8").tobytes()
        ch.observe_hashes(cap)
        fri.fold(ch.get_n_challenges(2))
    final = fri.final_poly()
    ch.observe_elements(final)
    witness = p.pow_grind(*ch.state(), case.params.proof_of_work_bits, ctx=ctx)
    ch.observe_elements([witness])
    assert ch.get_n_challenges(1)[0] >> (64 - case.params.proof_of_work_bits) == 0
    N = 1 << (case.params.degree_bits + case.params.rate_bits)
    x_index = [ch.get_n_challenges(1)[0] % N for _ in range(case.params.num_query_rounds)]
    out += fri.query(x_index) + np.ascontiguousarray(final, dtype="<u8").tobytes() + int(witness).to_bytes(8, "little")
    assert out == case.proof


@pytest.mark.gpu
def test_prover_calls_refuse_what_they_cannot_do(gpu):
    p, ctx = gpu
    case = stark_case(gpu, 7)
    def status(params, instance, batches):
        with pytest.raises(p.Plonky2Mi355xError) as e:
            p.PolynomialBatch.prove_openings(instance, batches, case.challenger(p), params, ctx=ctx)
        with pytest.raises(p.Plonky2Mi355xError) as e2:
            p.FriProver.from_instance(instance, batches, (1, 2), params, ctx=ctx)
        assert e.value.code == e2.value.code
        return e.value.code
    assert status(p.FriParams(7, 1, 4, 16, 84, [3]), case.instance, case.batches) == GL_ERR_UNSUPPORTED       # arity 8: as for circuits
    assert status(p.FriParams(7, 1, 4, 16, 84, [9]), case.instance, case.batches) == GL_ERR_ARG
    assert status(p.FriParams(8, 1, 4, 16, 84, [4]), case.instance, case.batches) == GL_ERR_ARG               # the batches' n
    assert status(p.FriParams(7, 2, 4, 16, 84, [4]), case.instance, case.batches) == GL_ERR_ARG               # rate_bits
    assert status(p.FriParams(7, 1, 3, 16, 84, [4]), case.instance, case.batches) == GL_ERR_ARG               # cap_height
    assert status(p.FriParams(7, 1, 4, 16, 84, [4], hasher="keccak"), case.instance, case.batches) == GL_ERR_ARG
    hiding = p.FriParams(7, 1, 4, 16, 84, [4], hiding=True)
    assert status(hiding, stark_instance(p, 7, (5, 6), blinding=(True, False, False)), case.batches) == GL_ERR_ARG            # salt expected, none there
    assert status(case.params, case.instance, case.batches[::-1]) == GL_ERR_ARG                                # column counts
    on_coset = (7 * pow(primitive_root(8), 5, P) % P, 0)
    assert status(case.params, stark_instance(p, 7, on_coset), case.batches) == GL_ERR_ARG


# ------------------------------------------------------------------------------- E: the tamper matrix
def tamper_case(gpu, orc, lg_n=7):
    case = stark_case(gpu, lg_n)
    if not hasattr(case, "trace"):
        case.trace = {}
        assert case.model(orc, max_queries=1, trace=case.trace) == fm.ACCEPTED
    return case, Layout(case.params, case.instance), case.trace["x_indices"][0]


# (name, n's log, byte to flip in query 0, code).  At n = 2^7 the one step tree has 16 leaves under a cap of 16: its paths are empty, so the
# step sibling is flipped in the n = 2^11 proof of C (256 leaves, four siblings).
EXACT = ([("leaf word of oracle %d" % o, 7, lambda lay, x, o=o: lay.leaf[o] + 8 * (lay.leaf_len[o] - 1), fm.INITIAL_MERKLE) for o in range(3)] + [
    ("initial sibling", 7, lambda lay, x: lay.sibling[2] + 32 + 8, fm.INITIAL_MERKLE),
    ("evals[x & 15] of the step", 7, lambda lay, x: lay.step_evals[0] + 16 * (x & 15), fm.FRI_CONSISTENCY),
    ("another eval of the same step leaf", 7, lambda lay, x: lay.step_evals[0] + 16 * ((x + 5) & 15) + 8, fm.STEP_MERKLE),
    ("step sibling", 11, lambda lay, x: lay.step_sibling[0] + 32 + 16, fm.STEP_MERKLE)])


@pytest.mark.gpu
@pytest.mark.parametrize("name,lg_n,where,code", EXACT, ids=[e[0] for e in EXACT])
def test_tampering_outside_the_transcript_names_the_check(gpu, orc, name, lg_n, where, code):
    p, ctx = gpu
    case, lay, x = tamper_case(gpu, orc, lg_n)
    assert lay.query0 < where(lay, x) < lay.query0 + lay.query_len
    bad = flip(case.proof, where(lay, x), bit=3)
    ok, why, got = case.library(p, proof=bad)
    assert (ok, got) == (False, code) and why.startswith(p.api.lib.gl_verify_check_message(code).decode())      # (the text, then file:line)
    assert case.model(orc, proof=bad, max_queries=1) == code


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["opening value", "oracle cap", "commit cap", "final coefficient", "PoW witness"])
def test_tampering_inside_the_transcript_is_rejected_as_the_model_says(gpu, orc, what):
    p, ctx = gpu
    case, lay, x = tamper_case(gpu, orc)
    kw = {}
    if what == "opening value":
        kw["openings"] = case.openings.copy()
        kw["openings"][5, 1] ^= U64(1 << 9)
    elif what == "oracle cap":
        kw["caps"] = case.caps.copy()
        kw["caps"][1, 3, 2] ^= U64(4)
    else:
        kw["proof"] = flip(case.proof, {"commit cap": lay.commit_caps + 40, "final coefficient": lay.final + 24, "PoW witness": lay.pow}[what], bit=1)
    want = case.model(orc, **kw)
    assert want != fm.ACCEPTED
    ok, why, got = case.library(p, **kw)
    assert (ok, got) == (False, want) and why


@pytest.mark.gpu
def test_truncation_and_trailing_bytes(gpu, orc):
    p, ctx = gpu
    case, lay, x = tamper_case(gpu, orc)
    for bad, code in ((case.proof[:-1], fm.TRUNCATED), (case.proof + b"\0", fm.LENGTH)):
        assert case.library(p, proof=bad)[0::2] == (False, code) and case.model(orc, proof=bad) == code
    wrong_length = bytearray(case.proof)
    wrong_length[lay.sibling[0] - 1] += 1                                        # an initial path one sibling longer: the decode runs off its end
    assert case.library(p, proof=bytes(wrong_length))[2] == case.model(orc, proof=bytes(wrong_length)) != fm.ACCEPTED


# ------------------------------------------------------------------------------- F: the committed proof (CPU)
def load_fixture(p):
    with open(os.path.join(GOLDEN, "fri_openings_n128.json")) as f:
        j = json.load(f)
    with open(os.path.join(GOLDEN, "fri_openings_n128.bin"), "rb") as f:
        proof = f.read()
    pr = j["params"]
    params = p.FriParams(pr["degree_bits"], pr["rate_bits"], pr["cap_height"], pr["proof_of_work_bits"], pr["num_query_rounds"], pr["reduction_arity_bits"],
                         hiding=pr["hiding"], hasher=pr["hasher"])
    instance = p.FriInstance([tuple(o) for o in j["oracles"]], [(tuple(pt), [tuple(oc) for oc in polys]) for pt, polys in j["batches"]])
    return params, instance, np.array(j["caps"], dtype=U64), np.array(j["openings"], dtype=U64), proof


def fixture_verdicts(p, orc, params, instance, caps, openings, proof):
    got = p.verify_fri_proof(instance, caps, openings, library_challenger(p, "poseidon", caps, openings), proof, params)
    want = fm.verify(params, instance, caps, openings, absorb(poseidon_challenger(orc), caps, openings), proof, fm.poseidon_verify_path(orc))
    return got, want


def test_fixture_is_accepted_and_64_bit_flips_are_rejected_by_both_verifiers(orc):
    import plonky2_demo_amd as p
    params, instance, caps, openings, proof = load_fixture(p)
    assert (params.degree_bits, params.rate_bits, params.cap_height, params.proof_of_work_bits, params.num_query_rounds) == (7, 1, 4, 16, 28)
    assert [k for k, _ in instance.oracles] == STARK_WIDTHS and [len(polys) for _, polys in instance.batches] == [13, 9]
    lay = Layout(params, instance)
    assert len(proof) == lay.size
    assert fixture_verdicts(p, orc, params, instance, caps, openings, proof) == ((True, "", 0), fm.ACCEPTED)
    rng = np.random.default_rng(2026)
    for k in range(64):
        bit = int(rng.integers(0, 64))
        if k % 2:                                                                # a bit of the final polynomial
            bad_proof, bad_openings = flip(proof, lay.final + int(rng.integers(0, lay.pow - lay.final)), bit % 8), openings
        else:                                                                    # a bit of an opening
            bad_proof, bad_openings = proof, openings.copy()
            bad_openings.reshape(-1)[int(rng.integers(0, openings.size))] ^= U64(1 << bit)
        (ok, why, got), want = fixture_verdicts(p, orc, params, instance, caps, bad_openings, bad_proof)
        assert not ok and why and got == want != fm.ACCEPTED, (k, got, want)


# ------------------------------------------------------------------------------- G: validation (CPU)
class TinyProof:
    """A FriProof assembled by hand: one oracle holding the constant polynomial c, opened at one point.  Its quotient is zero, so the
    codeword, its one reduction and the final polynomial are zero; every leaf of the initial tree is [c], every node of a level the
    same hash.  n = 8, rate_bits 1, cap_height 1, one reduction of arity 8 (arity bits 3), two queries, no proof of work."""

    def __init__(self, p, orc):
        self.p, c = p, 0x1234567
        self.params = p.FriParams(3, 1, 1, 0, 2, [3])
        self.instance = p.FriInstance([(1, False)], [((5, 0), [(0, 0)])])
        level = [orc.hash_or_noop([c])]
        for _ in range(3):
            level.append(orc.two_to_one(level[-1], level[-1]))
        step_leaf = orc.hash_or_noop(np.zeros(16, dtype=U64))
        self.caps = np.array([[level[3], level[3]]], dtype=U64)
        self.openings = np.array([[c, 0]], dtype=U64)
        words = lambda a: np.ascontiguousarray(np.asarray(a, dtype="<u8")).tobytes()      # noqa: E731
        query = words([c]) + bytes([3]) + words(level[:3]) + words(np.zeros(16, dtype=U64)) + bytes([0])
        self.proof = words([step_leaf, step_leaf]) + 2 * query + words([0, 0]) + words([0])

    def challenger(self, hasher="poseidon"):
        return library_challenger(self.p, hasher, self.caps, self.openings)

    def verify(self, params=None, instance=None, proof=None, challenger=None):
        # (longer arrays than the library reads: the binding holds their lengths against params that a refused case has changed)
        caps, openings = np.concatenate([self.caps.reshape(-1), np.zeros(256, dtype=U64)]), np.concatenate([self.openings.reshape(-1), np.zeros(16, dtype=U64)])
        return self.p.verify_fri_proof(instance or self.instance, caps, openings, challenger or self.challenger(), self.proof if proof is None else proof,
                                       params or self.params)


def test_a_reduction_of_arity_8_is_verified_on_its_merits(orc):
    import plonky2_demo_amd as p
    t = TinyProof(p, orc)
    assert t.verify() == (True, "", 0)
    model = lambda proof: fm.verify(t.params, t.instance, t.caps, t.openings, absorb(poseidon_challenger(orc), t.caps, t.openings), proof,      # noqa: E731
                                    fm.poseidon_verify_path(orc))
    assert model(t.proof) == fm.ACCEPTED
    lay = Layout(t.params, t.instance)
    for where in (lay.leaf[0], lay.step_evals[0] + 8, lay.final):
        bad = flip(t.proof, where)
        ok, why, code = t.verify(proof=bad)                                      # rejected with a check's code: never refused as unsupported
        assert not ok and code == model(bad) != fm.ACCEPTED


def _arg_cases(p):
    on_coset = 7 * pow(primitive_root(4), 3, P) % P
    def params(**kw):
        base = dict(degree_bits=3, rate_bits=1, cap_height=1, proof_of_work_bits=0, num_query_rounds=2, reduction_arity_bits=[3])
        extra = {k: kw.pop(k) for k in ("hiding_raw", "hasher_raw", "rounds_raw") if k in kw}
        base.update(kw)
        fp = p.FriParams(**base)
        for k, v in extra.items():
            setattr(fp, {"hiding_raw": "hiding", "hasher_raw": "hasher", "rounds_raw": "num_fri_rounds"}[k], v)
        return fp
    def instance(oracles=((1, False),), batches=(((5, 0), [(0, 0)]),), **raw):
        fi = p.FriInstance(list(oracles), list(batches))
        for k, v in raw.items():
            if k == "null_polys":
                fi.polys = ctypes.POINTER(ctypes.c_uint32)()
            elif k == "batch_len0":
                fi.batch_len[0] = v
            elif k == "blinding0":
                fi.oracle_blinding[0] = v
            elif k == "num_polys0":
                fi.oracle_num_polys[0] = v
            else:
                setattr(fi, k, v)
        return fi
    return [
        ("num_oracles 0", {"instance": instance(num_oracles=0)}), ("num_oracles 9", {"instance": instance(num_oracles=9)}),
        ("num_batches 0", {"instance": instance(num_batches=0)}), ("num_batches 5", {"instance": instance(num_batches=5)}),
        ("an empty batch", {"instance": instance(batch_len0=0)}), ("polys == NULL", {"instance": instance(null_polys=1)}),
        ("an oracle without polynomials", {"instance": instance(num_polys0=0)}), ("blinding 2", {"instance": instance(blinding0=2)}),
        ("oracle_index out of range", {"instance": instance(batches=[((5, 0), [(1, 0)])])}),
        ("polynomial_index out of range", {"instance": instance(batches=[((5, 0), [(0, 1)])])}),
        ("a point on the LDE coset", {"instance": instance(batches=[((on_coset, 0), [(0, 0)])])}),
        ("the coset's shift itself, non-canonical", {"instance": instance(batches=[((P + 7, P), [(0, 0)])])}),
        ("degree_bits 0", {"params": params(degree_bits=0, reduction_arity_bits=[])}),
        ("an LDE above 2^24", {"params": params(degree_bits=24)}),
        ("cap_height above the LDE", {"params": params(cap_height=5, reduction_arity_bits=[])}),
        ("arity bits 0", {"params": params(reduction_arity_bits=[0])}), ("arity bits 9", {"params": params(degree_bits=12, reduction_arity_bits=[9])}),
        ("nine reductions", {"params": params(degree_bits=12, reduction_arity_bits=[1] * 8, rounds_raw=9)}),
        ("a reduction below one coefficient", {"params": params(rate_bits=3, reduction_arity_bits=[2, 2])}),
        ("a reduction below the cap (circuit_builder.rs:977-980)", {"params": params(cap_height=2)}),
        ("no query round", {"params": params(num_query_rounds=0)}), ("257 query rounds", {"params": params(num_query_rounds=257)}),
        ("41 bits of work", {"params": params(proof_of_work_bits=41)}),
        ("hasher 2", {"params": params(hasher_raw=2)}), ("hiding 2", {"params": params(hiding_raw=2)}),
        ("a challenger under the other hasher", {"challenger": "keccak"}),
    ]


def test_validation_table(orc):
    import plonky2_demo_amd as p
    t = TinyProof(p, orc)
    for name, kw in _arg_cases(p):
        if "challenger" in kw:
            kw = {"challenger": p.Challenger(kw["challenger"])}
        with pytest.raises(p.Plonky2Mi355xError) as e:
            t.verify(**kw)
        assert e.value.code == GL_ERR_ARG, (name, str(e.value))
    # null pointers, through the binding itself
    lib, ch, buf, code = p.api.lib, t.challenger(), np.frombuffer(t.proof, dtype=np.uint8), ctypes.c_uint32()
    good = [ctypes.byref(t.params), ctypes.byref(t.instance), t.caps.ctypes.data, t.openings.ctypes.data, ch.handle, buf.ctypes.data, buf.size, ctypes.byref(code)]
    for k in range(6):
        args = list(good)
        args[k] = None
        assert lib.gl_verify_openings(*args) == GL_ERR_ARG, k
    good[7] = None                                                               # `check` may be null
    assert lib.gl_verify_openings(*good) == 0
    assert t.verify() == (True, "", 0)
