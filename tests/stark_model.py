"""A plain Python-integer model of the STARK prover's two own phases and of its verifier (no tests here), written from the reference:
  starky/src/permutation.rs:66-117,228-249    permutation_zs       the Z polynomials, get_permutation_batches' indexing literally
  constraint_consumer.rs:33-77,
  vanishing_poly.rs, permutation.rs:262-321   eval_vanishing       the consumer over the term list, then the permutation checks
  prover.rs:198-318                           quotient_values      (sum alpha^i C_i) / Z_H at every point of the quotient coset
  proof.rs:129-183, get_challenges.rs:21-73,
  verifier.rs:21-145,221-228                  parse / verify       the model verifier over the proof's bytes
The oracle library serves transforms, hashing and Merkle trees only; the transcript is transcript.DuplexChallenger and the FRI part
fri_openings_model.verify.  An AIR is one of stark_airs.py (constraints as term lists); field elements are Python integers, an
extension element a pair.  `Base` and `Ext` are the two fields the same consumer runs over.
"""
from types import SimpleNamespace

import numpy as np

import fri_openings_model as fom
from fri_openings_model import _ext_add, _ext_inv, _ext_sub
from stark_airs import ALL, FIRST_ROW, LAST_ROW, LOCAL, NEXT, PUBLIC, TRANSITION
from vanishing_model import P, _ext_mul, primitive_root

U64 = np.uint64
VANISHING = fom.VANISHING


class Base:
    zero, one = 0, 1
    lift = staticmethod(lambda v: int(v) % P)
    add = staticmethod(lambda a, b: (a + b) % P)
    sub = staticmethod(lambda a, b: (a - b) % P)
    mul = staticmethod(lambda a, b: a * b % P)


class Ext:
    zero, one = (0, 0), (1, 0)
    lift = staticmethod(lambda v: (int(v) % P, 0))
    add = staticmethod(_ext_add)
    sub = staticmethod(_ext_sub)
    mul = staticmethod(_ext_mul)


def num_zs(air, nc):
    return -(-len(air.pairs) * nc // air.q)                              # stark.rs:216-221


def permutation_batches(air, nc):
    """get_permutation_batches (permutation.rs:228-249): pairs x 0..num_challenges, chunked by q; instance i OF A CHUNK takes
    challenge_sets[i].challenges[chal] -> [[(pair index, set index, challenge index), ...], ...]"""
    instances = [(pair, chal) for pair in range(len(air.pairs)) for chal in range(nc)]
    return [[(pair, i, chal) for i, (pair, chal) in enumerate(instances[s:s + air.q])] for s in range(0, len(instances), air.q)]


def permutation_num_den(air, nc, trace, sets):
    """per Z polynomial the elementwise products of the reduced lhs and rhs columns (compute_permutation_z_poly, permutation.rs:91-102)"""
    n = len(trace[0])
    trace = [[int(v) % P for v in col] for col in trace]
    out = []
    for batch in permutation_batches(air, nc):
        num, den = [1] * n, [1] * n
        for pair, j, chal in batch:
            beta, gamma = (int(v) % P for v in sets[j][chal])
            lhs, rhs, weight = [gamma] * n, [gamma] * n, 1               # permutation_reduced_polys: gamma + sum beta^k column_k
            for a, b in air.pairs[pair]:
                lhs = [(x + weight * v) % P for x, v in zip(lhs, trace[a])]
                rhs = [(x + weight * v) % P for x, v in zip(rhs, trace[b])]
                weight = weight * beta % P
            num = [x * y % P for x, y in zip(num, lhs)]
            den = [x * y % P for x, y in zip(den, rhs)]
        out.append((num, den))
    return out


def permutation_zs(air, nc, trace, sets):
    """compute_permutation_z_polys: trace [num_columns][n]; sets[j][chal] = (beta, gamma) -> (Z values [nz][n], quotients [nz][n])"""
    zs, quotients = [], []
    for num, den in permutation_num_den(air, nc, trace, sets):
        assert all(den), "a permutation denominator is zero"
        quot = [x * pow(y, P - 2, P) % P for x, y in zip(num, den)]
        z, acc = [], 1
        for v in quot:
            z.append(acc)
            acc = acc * v % P
        zs.append(z)
        quotients.append(quot)
    return zs, quotients


def constraint_values(F, air, local, nxt, pub):
    """the Stark's own constraints, unfiltered: sum_t coeff_t prod_f operand_{t,f} over the field F"""
    out = []
    if F is Base:                                                        # the same sums with the arithmetic written in place: the quotient
        pub = [int(v) % P for v in pub]                                  # loop evaluates them at every point of the coset
        for _, terms in air.constraints:
            c = 0
            for coeff, ops in terms:
                m = coeff
                for kind, idx in ops:
                    m = m * (local[idx] if kind == LOCAL else nxt[idx] if kind == NEXT else pub[idx]) % P
                c += m
            out.append(c % P)
        return out
    for _, terms in air.constraints:
        c = F.zero
        for coeff, ops in terms:
            m = F.lift(coeff)
            for kind, idx in ops:
                m = F.mul(m, local[idx] if kind == LOCAL else nxt[idx] if kind == NEXT else F.lift(pub[idx]))
            c = F.add(c, m)
        out.append(c)
    return out


def eval_vanishing(F, air, nc, local, nxt, pub, alphas, z_last, l_first, l_last, zs_local=(), zs_next=(), sets=None):
    """eval_vanishing_poly through a ConstraintConsumer: the accumulators, one per alpha"""
    accs = [F.zero] * nc
    alphas = [F.lift(a) for a in alphas]

    def consume(c):                                                      # ConstraintConsumer::constraint
        for j in range(nc):
            accs[j] = F.add(F.mul(accs[j], alphas[j]), c)
    for (filt, _), c in zip(air.constraints, constraint_values(F, air, local, nxt, pub)):
        assert filt in (ALL, TRANSITION, FIRST_ROW, LAST_ROW)
        consume(c if filt == ALL else F.mul(c, {TRANSITION: z_last, FIRST_ROW: l_first, LAST_ROW: l_last}[filt]))
    if air.pairs:                                                        # eval_permutation_checks (permutation.rs:282-320)
        for z in zs_local:
            consume(F.mul(F.sub(z, F.one), l_first))
        for b, batch in enumerate(permutation_batches(air, nc)):
            lhs_prod, rhs_prod = zs_local[b], zs_next[b]
            for pair, j, chal in batch:
                beta, gamma = (F.lift(v) for v in sets[j][chal])
                lhs, rhs = F.zero, F.zero
                for a, c in reversed(air.pairs[pair]):                   # ReducingFactor::reduce_ext: sum beta^k value_k
                    lhs = F.add(F.mul(lhs, beta), local[a])
                    rhs = F.add(F.mul(rhs, beta), local[c])
                lhs_prod = F.mul(lhs_prod, F.add(lhs, gamma))
                rhs_prod = F.mul(rhs_prod, F.add(rhs, gamma))
            consume(F.sub(rhs_prod, lhs_prod))
    return accs


def lagrange_on_coset(orc, lg_n, qdb):
    """PolynomialValues::selector(n, 0 | n - 1).lde_onto_coset(qdb) (prover.rs:230-234), the reference's own way"""
    n = 1 << lg_n
    sel = np.zeros((2, n), dtype=U64)
    sel[0, 0] = sel[1, n - 1] = 1
    lde = orc.lde(orc.ifft(sel), qdb)
    return [int(v) for v in lde[0]], [int(v) for v in lde[1]]


def quotient_values(orc, air, nc, lg_n, trace_q, zs_q, sets, alphas, pub):
    """compute_quotient_polys before its coset_ifft: trace_q [num_columns][size], zs_q [nz][size] = the LDE values at the points 7 w^i of
    the quotient coset (size = n << qdb), natural order -> [nc][size]"""
    n, size = 1 << lg_n, (1 << lg_n) << air.qdb
    l_first, l_last = lagrange_on_coset(orc, lg_n, air.qdb)
    last = pow(primitive_root(lg_n), P - 2, P)
    w = primitive_root(lg_n + air.qdb)
    # rows once (a transpose), so that a point costs two list lookups, not one comprehension per column
    rows = np.asarray(trace_q, dtype=U64).T.tolist()
    z_rows = np.asarray(zs_q, dtype=U64).T.tolist() if len(zs_q) else [[]] * size
    out = [[0] * size for _ in range(nc)]
    x = 7
    for i in range(size):
        nx = (i + (1 << air.qdb)) % size
        accs = eval_vanishing(Base, air, nc, rows[i], rows[nx], pub, alphas, (x - last) % P, l_first[i], l_last[i], z_rows[i], z_rows[nx], sets)
        z_h_inv = pow((pow(x, n, P) - 1) % P, P - 2, P)
        for j in range(nc):
            out[j][i] = accs[j] * z_h_inv % P
        x = x * w % P
    return out


def quotient_chunks(orc, air, nc, lg_n, values):
    """values.coset_ifft(7), trim_to_len(q n), chunks(n) (prover.rs:123-131, 313-317) -> [nc * q][n], or None where the trim fails"""
    n = 1 << lg_n
    coeffs = orc.coset_ifft(np.array(values, dtype=U64), 7)
    if coeffs[:, air.q * n:].any():
        return None
    return coeffs[:, :air.q * n].reshape(nc * air.q, n)


def eval_ext_values(orc, values, z):
    """the polynomial through `values` on H at the extension point z"""
    from prover_phase_model import eval_ext
    return eval_ext(orc.ifft(np.array(values, dtype=U64)), z)


def ext_pow2(x, k):
    for _ in range(k):
        x = _ext_mul(x, x)
    return x


def l_first_last_at(lg_n, x):
    """eval_l_0_and_l_last (verifier.rs:221-228)"""
    n, g = (1 << lg_n) % P, primitive_root(lg_n)
    z_x = _ext_sub(ext_pow2(x, lg_n), (1, 0))
    a = _ext_inv(_ext_mul((n, 0), _ext_sub(x, (1, 0))))
    b = _ext_inv(_ext_mul((n, 0), _ext_sub(_ext_mul((g, 0), x), (1, 0))))
    return _ext_mul(z_x, a), _ext_mul(z_x, b)


def vanishing_at(air, nc, lg_n, zeta, local, nxt, pub, alphas, zs_local=(), zs_next=(), sets=None):
    """verifier.rs:81-106: the accumulators at zeta over the extension field"""
    l_first, l_last = l_first_last_at(lg_n, zeta)
    last = pow(primitive_root(lg_n), P - 2, P)
    return eval_vanishing(Ext, air, nc, local, nxt, pub, alphas, _ext_sub(zeta, (last, 0)), l_first, l_last, zs_local, zs_next, sets)


def identity_holds(air, nc, lg_n, zeta, vanishing, quotient_openings):
    """verifier.rs:108-124: vanishing_j == Z_H(zeta) reduce_with_powers(chunk_j, zeta^n) for every challenge"""
    zeta_pow = ext_pow2(zeta, lg_n)
    z_h = _ext_sub(zeta_pow, (1, 0))
    for j in range(nc):
        acc = (0, 0)
        for t in reversed(quotient_openings[j * air.q:(j + 1) * air.q]):
            acc = _ext_add(_ext_mul(acc, zeta_pow), t)
        if vanishing[j] != _ext_mul(z_h, acc):
            return False
    return True


# ------------------------------------------------------------------------------- the proof's bytes and the model verifier
def fri_instance(air, nc, zeta, lg_n):
    """stark.rs:88-137 as fri_openings_model takes it"""
    nz, g = num_zs(air, nc), primitive_root(lg_n)
    oracles = [(air.num_columns, False)] + ([(nz, False)] if nz else []) + [(air.q * nc, False)]
    trace = [(0, c) for c in range(air.num_columns)]
    zs = [(1, c) for c in range(nz)]
    quotient = [(len(oracles) - 1, c) for c in range(air.q * nc)]
    zeta = (int(zeta[0]) % P, int(zeta[1]) % P)
    return SimpleNamespace(oracles=oracles, batches=[(zeta, trace + zs + quotient), ((zeta[0] * g % P, zeta[1] * g % P), trace + zs)])


def fri_proof_size(params, instance):
    """the size gl_prove_openings' bytes have: fixed by the params and the instance"""
    hash_bytes = 25 if params.hasher else 32
    lgN, size = params.degree_bits + params.rate_bits, 0
    size += len(params.reduction_arity_bits) * (hash_bytes << params.cap_height)
    per_query, lg = 0, lgN
    for k, _ in instance.oracles:
        per_query += 8 * k + 1 + hash_bytes * (lgN - params.cap_height)
    for ab in params.reduction_arity_bits:
        lg -= ab
        per_query += 16 * (1 << ab) + 1 + hash_bytes * (lg - params.cap_height)
    size += params.num_query_rounds * per_query
    return size + 16 * ((1 << params.degree_bits) >> sum(params.reduction_arity_bits)) + 8


class ParsedStarkProof:
    """The layout of include/plonky2_mi355x.h: trace_cap, permutation_zs_cap (with pairs), quotient_polys_cap, local_values, next_values,
    permutation_zs and permutation_zs_next (with pairs), quotient_polys (two words each), the FriProof, the public inputs."""

    def __init__(self, air, nc, params, by):
        self.by, self.pos, self.keccak = bytes(by), 0, bool(params.hasher)
        nz, ncap = num_zs(air, nc), 1 << params.cap_height
        self.trace_cap = self.hashes(ncap)
        self.zs_cap = self.hashes(ncap) if nz else None
        self.quotient_cap = self.hashes(ncap)
        self.local, self.next = self.exts(air.num_columns), self.exts(air.num_columns)
        self.zs, self.zs_next = (self.exts(nz), self.exts(nz)) if nz else ([], [])
        self.quotient = self.exts(air.q * nc)
        fri_len = fri_proof_size(params, fri_instance(air, nc, (0, 1), params.degree_bits))
        tail = 8 * air.num_public_inputs
        if len(self.by) - self.pos < fri_len + tail:
            raise fom.Malformed(fom.TRUNCATED)
        if len(self.by) - self.pos > fri_len + tail:
            raise fom.Malformed(fom.LENGTH)
        self.fri = self.take(fri_len)
        self.public_inputs = self.words(air.num_public_inputs)

    def take(self, k):
        if self.pos + k > len(self.by):
            raise fom.Malformed(fom.TRUNCATED)
        self.pos += k
        return self.by[self.pos - k:self.pos]

    def words(self, k):
        return [int.from_bytes(self.take(8), "little") % P for _ in range(k)]

    def exts(self, k):
        w = self.words(2 * k)
        return [(w[2 * i], w[2 * i + 1]) for i in range(k)]

    def hashes(self, k):
        if self.keccak:
            return [[int.from_bytes(b[i:i + 8], "little") for i in range(0, 32, 8)] for b in (self.take(25).ljust(32, b"\0") for _ in range(k))]
        return [self.words(4) for _ in range(k)]

    def fri_openings(self):
        """to_fri_openings (proof.rs:161-182): [local, zs, quotient] at zeta, then [next, zs_next] at g zeta"""
        return self.local + self.zs + self.quotient + self.next + self.zs_next


def replay(air, nc, proof, challenger):
    """get_challenges.rs:21-59 up to the openings -> (challenge sets or None, alphas, zeta)"""
    challenger.observe_hashes(np.array(proof.trace_cap, dtype=U64))
    sets = None
    if air.pairs:
        sets = [[tuple(challenger.get(2)) for _ in range(nc)] for _ in range(air.q)]      # (beta, gamma) per challenge, set after set
        challenger.observe_hashes(np.array(proof.zs_cap, dtype=U64))
    alphas = challenger.get(nc)
    challenger.observe_hashes(np.array(proof.quotient_cap, dtype=U64))
    zeta = tuple(challenger.get(2))
    challenger.observe(np.array(proof.fri_openings(), dtype=U64))
    return sets, alphas, zeta


def verify(air, nc, params, by, challenger, verify_path, max_queries=None, trace=None):
    """verify_stark_proof (verifier.rs:21-145) -> the GL_CHECK_* code of the first failing check (0: accepted)"""
    try:
        proof = ParsedStarkProof(air, nc, params, by)
    except fom.Malformed as e:
        return e.code
    sets, alphas, zeta = replay(air, nc, proof, challenger)
    if trace is not None:
        trace.update(stark_proof=proof, sets=sets, alphas=alphas, zeta=zeta)
    vanishing = vanishing_at(air, nc, params.degree_bits, zeta, proof.local, proof.next, proof.public_inputs, alphas, proof.zs, proof.zs_next, sets)
    if not identity_holds(air, nc, params.degree_bits, zeta, vanishing, proof.quotient):
        return VANISHING
    caps = [proof.trace_cap] + ([proof.zs_cap] if air.pairs else []) + [proof.quotient_cap]
    return fom.verify(params, fri_instance(air, nc, zeta, params.degree_bits), np.array(caps, dtype=U64), np.array(proof.fri_openings(), dtype=U64),
                      challenger, proof.fri, verify_path, max_queries=max_queries, trace=trace)
