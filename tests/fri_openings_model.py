"""A plain Python-integer model of FRI openings for any FriInstanceInfo (no tests here).

Two parts, both written from the reference:
  fri/oracle.rs:162-219, util/reducing.rs:83-106     final_poly       prove_openings' loop over the batches, literally, with the
                                                                      ReducingFactor's shared counter (gl_fri_combine_instance)
  fri/verifier.rs:21-260, fri/challenges.rs:24-64,
  fri/validate_shape.rs, hash/merkle_proofs.rs:54-75 verify           verify_fri_proof over the parsed FriProof (gl_verify_openings)
The verifier hashes through what it is given (`verify_path`: the oracle library's Merkle check under Poseidon, the Keccak model of
test_keccak.py under Keccak) and draws its challenges from a transcript.DuplexChallenger, so the transcript order is pinned by something
that is not the library's challenger.  It answers with the library's GL_CHECK_* numbers, in the library's documented order.

`params` needs the attributes degree_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, reduction_arity_bits, hiding,
hasher; `instance` needs oracles = [(num_polys, blinding)] and batches = [(point, [(oracle_index, polynomial_index)])].
"""
import numpy as np

from prover_phase_model import divide_by_linear, eval_ext, fold, reduce_polys_base      # noqa: F401  (eval_ext, fold: for the tests)
from vanishing_model import P, _ext_mul, primitive_root

U64 = np.uint64
SALT_SIZE = 4
(ACCEPTED, VERIFIER_DATA, STEP_PATH_LENGTH, INITIAL_PATH_LENGTH, TRUNCATED, PUBLIC_INPUT_COUNT, LENGTH, VANISHING, POW, INITIAL_MERKLE,
 FRI_CONSISTENCY, STEP_MERKLE, FINAL_POLY) = range(13)


def _ext(z):
    return (int(z[0]) % P, int(z[1]) % P)


def _ext_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def _ext_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def _ext_inv(x):
    """1 / (a + b X) = (a - b X) / (a^2 - 7 b^2) in F_p[X] / (X^2 - 7)"""
    norm = (x[0] * x[0] - 7 * x[1] * x[1]) % P
    assert norm, "inverse of zero"
    k = pow(norm, P - 2, P)
    return (x[0] * k % P, -x[1] * k % P)


def _ext_pow(x, e):
    r = (1, 0)
    for _ in range(e):
        r = _ext_mul(r, x)
    return r


def _reverse_bits(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ------------------------------------------------------------------------------- prove_openings up to fri_proof
def final_poly(instance, columns, alpha):
    """prove_openings (oracle.rs:183-197): columns[oracle][polynomial] = n base-field coefficients -> the n extension coefficients of
    final_poly.  The ReducingFactor counts the polynomials reduce_polys_base took; shift_poly multiplies by alpha^count and resets it."""
    alpha, count = _ext(alpha), 0
    final = None                                                                # PolynomialCoeffs::empty()
    for point, polys in instance.batches:
        composition = reduce_polys_base([[int(v) for v in columns[o][c]] for o, c in polys], alpha)
        count += len(polys)                                                     # reducing.rs:88
        quotient = divide_by_linear(composition, point) + [(0, 0)]              # quotient.coeffs.push(ZERO)
        shift = _ext_pow(alpha, count)                                          # shift_poly: *p *= base^count; count = 0
        count = 0
        final = quotient if final is None else [_ext_add(_ext_mul(f, shift), q) for f, q in zip(final, quotient)]
    return final


def openings_of(instance, columns):
    """FriOpenings: per batch the values of its polynomials at its point, batch after batch -> [k][2]"""
    return [eval_ext(columns[o][c], point) for point, polys in instance.batches for o, c in polys]


# ------------------------------------------------------------------------------- the FriProof's bytes
class Malformed(Exception):
    def __init__(self, code):
        super().__init__("malformed proof: %d" % code)
        self.code = code


class ParsedFriProof:
    """write_fri_proof (util/serialization/mod.rs:1568-1582): commit-phase caps, query rounds, final polynomial, PoW witness.  Field words
    are taken mod p as read_field does; a hash is four words under Poseidon, 25 bytes in a four-word slot under Keccak."""

    def __init__(self, params, instance, by):
        self.by, self.pos, self.keccak = bytes(by), 0, bool(params.hasher)
        arity = list(params.reduction_arity_bits)
        lgN, ncap = params.degree_bits + params.rate_bits, 1 << params.cap_height
        self.leaf_lens = [k + (SALT_SIZE if params.hiding and blinding else 0) for k, blinding in instance.oracles]
        self.commit_caps = [self.hashes(ncap) for _ in arity]
        self.queries = []
        for _ in range(params.num_query_rounds):
            init, steps, lg = [], [], lgN
            for k in self.leaf_lens:
                leaf = self.words(k)
                init.append((leaf, self.hashes(self.u8())))
            for ab in arity:
                evals = self.words(2 << ab)
                lg -= ab
                steps.append((evals, self.hashes(self.u8())))
                if len(steps[-1][1]) != lg - params.cap_height:
                    raise Malformed(STEP_PATH_LENGTH)
            if any(len(sib) != lgN - params.cap_height for _, sib in init):
                raise Malformed(INITIAL_PATH_LENGTH)
            self.queries.append((init, steps))
        self.final_poly = self.words(2 * ((1 << params.degree_bits) >> sum(arity)))
        self.pow_witness = self.words(1)[0]
        if self.pos != len(self.by):
            raise Malformed(LENGTH)

    def take(self, k):
        if self.pos + k > len(self.by):
            raise Malformed(TRUNCATED)
        self.pos += k
        return self.by[self.pos - k:self.pos]

    def u8(self):
        return self.take(1)[0]

    def words(self, k):
        return [int.from_bytes(self.take(8), "little") % P for _ in range(k)]

    def hashes(self, k):
        if self.keccak:
            return [[int.from_bytes(b[i:i + 8], "little") for i in range(0, 32, 8)] for b in (self.take(25).ljust(32, b"\0") for _ in range(k))]
        return [self.words(4) for _ in range(k)]


# ------------------------------------------------------------------------------- verify_fri_proof
def compute_evaluation(x, x_index_within_coset, arity_bits, evals, beta):
    """fri/verifier.rs:21-47: the evaluations (bit-reversed order) interpolated over the coset of x, at beta"""
    arity = 1 << arity_bits
    g = primitive_root(arity_bits)
    evals = [evals[_reverse_bits(i, arity_bits)] for i in range(arity)]          # reverse_index_bits_in_place
    coset_start = x * pow(g, arity - _reverse_bits(x_index_within_coset, arity_bits), P) % P
    points = [coset_start * pow(g, i, P) % P for i in range(arity)]
    acc = (0, 0)
    for i, (xi, yi) in enumerate(zip(points, evals)):                            # interpolate: Lagrange form
        num, den = (1, 0), 1
        for j, xj in enumerate(points):
            if j != i:
                num = _ext_mul(num, _ext_sub(beta, (xj, 0)))
                den = den * (xi - xj) % P
        k = pow(den, P - 2, P)
        acc = _ext_add(acc, _ext_mul(yi, (num[0] * k % P, num[1] * k % P)))
    return acc


def verify(params, instance, caps, openings, challenger, by, verify_path, max_queries=None, trace=None):
    """-> the GL_CHECK_* code of the first failing check (0: accepted).  caps [num_oracles][2^cap_height][4]; openings [k][2] in batch
    order; `challenger`: a transcript.DuplexChallenger in the state after the openings were observed; verify_path(leaf, index, cap,
    siblings) -> bool.  max_queries: check only the first that many query rounds (all challenges are drawn regardless); trace: a
    dict that receives the parsed proof and the challenges drawn."""
    try:
        proof = ParsedFriProof(params, instance, by)
    except Malformed as e:
        return e.code
    arity = list(params.reduction_arity_bits)
    lgN = params.degree_bits + params.rate_bits
    N = 1 << lgN
    # fri/challenges.rs:24-64
    alpha = _ext(challenger.get(2))
    betas = []
    for cap in proof.commit_caps:
        challenger.observe_hashes(np.array(cap, dtype=U64))
        betas.append(_ext(challenger.get(2)))
    challenger.observe(np.array(proof.final_poly, dtype=U64))
    challenger.observe([proof.pow_witness])
    pow_response = challenger.get(1)[0]
    x_indices = [challenger.get(1)[0] % N for _ in range(params.num_query_rounds)]
    if trace is not None:
        trace.update(proof=proof, alpha=alpha, betas=betas, pow_response=pow_response, x_indices=x_indices)
    # fri_verify_proof_of_work (verifier.rs:49-60): leading_zeros of the canonical u64
    if params.proof_of_work_bits and pow_response >> (64 - params.proof_of_work_bits):
        return POW
    # PrecomputedReducedOpenings (verifier.rs:243-260): ReducingFactor::reduce = sum_j alpha^j value_j per batch
    openings = [_ext(v) for v in np.asarray(openings, dtype=U64).reshape(-1, 2)]
    reduced, at = [], 0
    for _, polys in instance.batches:
        acc = (0, 0)
        for v in reversed(openings[at:at + len(polys)]):
            acc = _ext_add(_ext_mul(acc, alpha), v)
        reduced.append(acc)
        at += len(polys)
    caps = np.asarray(caps, dtype=U64).reshape(len(instance.oracles), -1, 4)
    for x_index, (init, steps) in list(zip(x_indices, proof.queries))[:max_queries]:
        # fri_verify_initial_proof (verifier.rs:110-120)
        for (leaf, siblings), cap in zip(init, caps):
            if not verify_path(leaf, x_index, cap, siblings):
                return INITIAL_MERKLE
        subgroup_x = 7 * pow(primitive_root(lgN), _reverse_bits(x_index, lgN), P) % P
        # fri_combine_initial (verifier.rs:122-161); unsalted_eval: the leaf without its last salt_size(salted) words
        total, count = (0, 0), 0
        for (point, polys), reduced_openings in zip(instance.batches, reduced):
            evals = []
            for o, c in polys:
                salted = bool(params.hiding and instance.oracles[o][1])
                leaf = init[o][0]
                evals.append(leaf[:len(leaf) - (SALT_SIZE if salted else 0)][c])
            acc = (0, 0)
            for v in reversed(evals):                                            # alpha.reduce(evals); count += len
                acc = _ext_add(_ext_mul(acc, alpha), (v, 0))
            count += len(evals)
            numerator = _ext_sub(acc, reduced_openings)
            denominator = _ext_sub((subgroup_x, 0), _ext(point))
            total = _ext_mul(total, _ext_pow(alpha, count))                      # alpha.shift(sum); count = 0
            count = 0
            total = _ext_add(total, _ext_mul(numerator, _ext_inv(denominator)))
        old_eval = total
        for i, ab in enumerate(arity):
            evals = [(steps[i][0][2 * k], steps[i][0][2 * k + 1]) for k in range(1 << ab)]
            coset_index, within = x_index >> ab, x_index & ((1 << ab) - 1)
            if evals[within] != old_eval:
                return FRI_CONSISTENCY
            old_eval = compute_evaluation(subgroup_x, within, ab, evals, betas[i])
            if not verify_path(steps[i][0], coset_index, proof.commit_caps[i], steps[i][1]):
                return STEP_MERKLE
            subgroup_x = pow(subgroup_x, 1 << ab, P)
            x_index = coset_index
        final = [(proof.final_poly[2 * k], proof.final_poly[2 * k + 1]) for k in range(len(proof.final_poly) // 2)]
        acc = (0, 0)
        for c in reversed(final):
            acc = _ext_add(_ext_mul(acc, (subgroup_x, 0)), c)
        if acc != old_eval:
            return FINAL_POLY
    return ACCEPTED


def poseidon_verify_path(orc):
    """verify_merkle_proof_to_cap (merkle_proofs.rs:54-75) by the oracle library's Poseidon"""
    def verify_path(leaf, index, cap, siblings):
        return orc.merkle_verify(np.array(leaf, dtype=U64), index, np.asarray(cap, dtype=U64) % U64(P), np.array(siblings, dtype=U64).reshape(-1, 4))
    return verify_path
