"""The Fiat-Shamir transcript as a caller of the phase-level ABI keeps it, shared by the tests (no tests here): one model of the duplex
Challenger, the same interface over the library's own, the replay of a parsed proof and the driver of the phase entry points."""
from types import SimpleNamespace

import numpy as np

from oracle_lib import P
from proof_parser import NUM_WIRES, NUM_ZS, NUM_ZS_PP, proof_bytes

U64 = np.uint64
# FriOpenings order (proof.rs:346-380): the batches at zeta, then the second batch's Z and lookup polynomials at g * zeta
FRI_OPENINGS = ("constants", "sigmas", "wires", "zs", "pp", "quotient", "lookups", "zs_next", "lookups_next")


class DuplexChallenger:
    """iop/challenger.rs:30-153 over `permute` (12 elements -> 12 elements); `hash_elements` maps [k][4] digest words to the field
    elements a hash of the configuration's Hasher is observed as.  A hash of C::InnerHasher (the public-input hash: Poseidon under both
    configurations) is observed as its own four elements."""

    def __init__(self, permute, hash_elements):
        self.permute, self.hash_elements = permute, hash_elements
        self.state, self.inp, self.out = [0] * 12, [], []

    def _duplex(self):
        self.state[:len(self.inp)] = self.inp
        self.inp = []
        self.state = [int(x) for x in self.permute(self.state)]
        self.out = self.state[:8]

    def observe(self, xs):
        for x in np.asarray(xs, dtype=U64).reshape(-1):
            self.out = []
            self.inp.append(int(x) % P)
            if len(self.inp) == 8:
                self._duplex()

    def observe_hashes(self, digests, inner=False):
        for h in np.asarray(digests, dtype=U64).reshape(-1, 4) if inner else self.hash_elements(digests):
            self.observe(h)

    def get(self, k):
        r = []
        for _ in range(k):
            if self.inp or not self.out:
                self._duplex()
            r.append(self.out.pop() % P)
        return r


def poseidon_challenger(orc):
    """The model over the oracle's Poseidon permutation; a HashOut is its four elements."""
    return DuplexChallenger(lambda s: orc.poseidon(np.array(s, dtype=U64)), lambda digests: np.asarray(digests, dtype=U64).reshape(-1, 4))


class LibraryChallenger:
    """The same interface over the library's own gl_challenger_* (for callers without a transcript implementation)."""

    def __init__(self, p, hasher="poseidon"):
        self.ch = p.Challenger(hasher=hasher)

    def observe(self, xs):
        self.ch.observe_elements(xs)

    def observe_hashes(self, digests, inner=False):
        self.ch.observe_hashes(digests, hasher="poseidon" if inner else None)

    def get(self, k):
        return self.ch.get_n_challenges(k)

    @property
    def state(self):
        return self.ch.state()[0]

    @property
    def inp(self):
        return self.ch.state()[1]


def public_inputs_hash(orc, pis):
    return orc.hash_no_pad(pis) if len(pis) else np.zeros(4, dtype=U64)


def replay_to_openings(d, ch, digest, pi_hash, pp):
    """prover.rs:158-227 of the parsed proof `pp` on the challenger `ch`, up to and including the observed openings: where the FriProof's
    own transcript starts (fri/prover.rs).  -> (betas, gammas, lookup deltas or None, alphas, zeta)"""
    ch.observe_hashes(digest)
    ch.observe_hashes(pi_hash, inner=True)
    ch.observe_hashes(pp.caps[0])
    betas, gammas = ch.get(2), ch.get(2)
    deltas = betas + gammas + ch.get(4) if d.num_lookup_polys else None           # prover.rs:166-184
    ch.observe_hashes(pp.caps[1])
    alphas = ch.get(2)
    ch.observe_hashes(pp.caps[2])
    zeta = ch.get(2)
    for name in FRI_OPENINGS:
        ch.observe(pp.openings[name])
    return betas, gammas, deltas, alphas, zeta


def replay_transcript(d, ch, digest, pi_hash, pp):
    """prover.rs:158-227,273,298 / fri/prover.rs:91-93,111,153 of the parsed proof `pp` on the challenger `ch`: (challenges as
    Proof.challenges() gives them, PoW response, query indices, lookup deltas or None).  The native verifier shares HostChallenger with the
    prover, so this replay on a model challenger is what pins the transcript."""
    betas, gammas, deltas, alphas, zeta = replay_to_openings(d, ch, digest, pi_hash, pp)
    fri_alpha = ch.get(2)
    fri_betas = []
    for cap in pp.fri_caps:
        ch.observe_hashes(cap)
        fri_betas.append(ch.get(2))
    ch.observe(pp.final_poly)
    ch.observe([pp.pow_witness])
    response = ch.get(1)[0]
    N = 1 << (d.degree_bits + d.rate_bits)
    x_index = [ch.get(1)[0] % N for _ in range(d.num_query_rounds)]
    return {"betas": betas, "gammas": gammas, "alphas": alphas, "zeta": zeta, "fri_alpha": fri_alpha, "pow_witness": pp.pow_witness,
            "public_inputs_hash": [int(x) for x in pi_hash], "fri_betas": fri_betas}, response, x_index, deltas


def drive_phase_api(p, ctx, orc, cd, ch, wires, pis):
    """Every phase entry point of include/plonky2_mi355x.h driven by the caller-side challenger `ch`, in the order of
    plonk/prover.rs:102-329, for a circuit with or without lookups under either hasher.  Circuits with lookups pass the delta challenges
    ([betas | gammas | 4 drawn after them], prover.rs:166-184), and their lookup polynomials are the last columns of the second batch.
    -> everything the caller saw, and the ProofWithPublicInputs bytes it assembled."""
    d = cd.desc
    n, N, nlp = 1 << d.degree_bits, 1 << (d.degree_bits + d.rate_bits), d.num_lookup_polys
    hasher = "keccak" if d.hasher else "poseidon"
    r = SimpleNamespace(pi_hash=public_inputs_hash(orc, pis), d_wires=ctx.alloc(wires.nbytes).upload(wires))
    ch.observe_hashes(cd.circuit_digest)
    ch.observe_hashes(r.pi_hash, inner=True)
    r.wires_b = p.PolynomialBatch.from_device(r.d_wires.ptr, NUM_WIRES, n, d.rate_bits, d.cap_height, True, ctx=ctx, hasher=hasher)
    ch.observe_hashes(r.wires_b.cap)
    r.betas, r.gammas = ch.get(2), ch.get(2)
    r.deltas = list(r.betas) + list(r.gammas) + list(ch.get(4)) if nlp else None
    r.zs_b = cd.partial_products(r.d_wires.ptr, r.betas, r.gammas, ctx=ctx, deltas=r.deltas)
    ch.observe_hashes(r.zs_b.cap)
    r.alphas = ch.get(2)
    r.q_b = cd.quotient_polys(r.wires_b, r.zs_b, r.pi_hash, r.betas, r.gammas, r.alphas, ctx=ctx, deltas=r.deltas)
    ch.observe_hashes(r.q_b.cap)
    r.zeta = ch.get(2)
    g = orc.primitive_root(d.degree_bits)
    r.gzeta = [r.zeta[0] * g % P, r.zeta[1] * g % P]
    r.batches = [cd.constants_sigmas_batch, r.wires_b, r.zs_b, r.q_b]
    o_cs, o_w, o_z, o_q = (b.open_at(r.zeta) for b in r.batches)
    r.openings = {"constants": o_cs[:d.num_constants], "sigmas": o_cs[d.num_constants:], "wires": o_w, "zs": o_z[:NUM_ZS],
                  "pp": o_z[NUM_ZS:NUM_ZS_PP], "quotient": o_q, "lookups": o_z[NUM_ZS_PP:], "zs_next": r.zs_b.open_at(r.gzeta, 0, NUM_ZS),
                  "lookups_next": r.zs_b.open_at(r.gzeta, NUM_ZS_PP, 2 * nlp) if nlp else o_z[:0]}
    for name in FRI_OPENINGS:
        ch.observe(r.openings[name])
    r.fri_alpha = ch.get(2)
    r.fri = cd.fri(r.batches, r.zeta, r.fri_alpha, ctx=ctx)
    r.fri_caps = []
    for _ in range(d.num_fri_rounds):
        r.fri_caps.append(r.fri.commit_round())
        ch.observe_hashes(r.fri_caps[-1])
        r.fri.fold(ch.get(2))
    r.final_poly = r.fri.final_poly()
    ch.observe(r.final_poly)
    r.pow_witness = p.pow_grind(ch.state, ch.inp, d.proof_of_work_bits, ctx=ctx, hasher=hasher)
    ch.observe([r.pow_witness])
    r.pow_response = ch.get(1)[0]
    assert r.pow_response >> (64 - d.proof_of_work_bits) == 0
    r.x_index = [ch.get(1)[0] % N for _ in range(d.num_query_rounds)]
    r.query_blob = r.fri.query(r.x_index)
    r.bytes = proof_bytes(d, [r.wires_b.cap, r.zs_b.cap, r.q_b.cap], r.openings, r.fri_caps, r.query_blob, r.final_poly, r.pow_witness, pis)
    return r
