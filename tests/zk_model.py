"""A whole zero-knowledge proof derived from plain integers (no tests here).

derive() follows prove_with_partition_witness (plonk/prover.rs:102-329) for a zero-knowledge circuit: every oracle but constants || sigmas
is a blinded PolynomialBatch (fri/oracle.rs:100-125: SALT_SIZE random words behind every leaf), the witness carries blind()'s rows
(circuit_builder.rs:777-818).  What computes what:
  the keystream, blind()'s layout, the salt          zk_circuits.py (ChaCha20 from RFC 8439, circuit_builder.rs:718-818)
  Z and the partial products                         prover_phase_model.partial_products
  the quotient                                       vanishing_model.vanishing_over_z_h at every LDE point, or vanishing_terms at chosen ones
  openings, batch reduction, division, folds         prover_phase_model.eval_ext, combine_and_divide, fold
  iFFT, LDE, coset FFT, Poseidon, Poseidon trees     the C++ oracle (oracle_lib)
  Keccak trees, transcript and proof of work         the numpy model of test_keccak.py
  the transcript                                     transcript.DuplexChallenger
  the bytes                                          proof_parser.proof_bytes
verify() is the verifier written the same way: the vanishing identity at zeta (plonk/verifier.rs:49-96, vanishing_poly.rs:54-161) with
vanishing_model's gate functions run on extension-field values, then fri_openings_model.verify with the blinded oracles marked.
Nothing here calls into the product.  `d` is the circuit description the caller hands in (a gl_circuit_desc or anything with its fields).
"""
import time
from types import SimpleNamespace

import numpy as np

import fri_openings_model as fm
import prover_phase_model as pm
import vanishing_model as vm
from oracle_lib import P
from proof_parser import NUM_QUOTIENT, NUM_SIGMAS, NUM_WIRES, NUM_ZS, NUM_ZS_PP, ParsedProof, hash_bytes, opening_columns, proof_bytes
from transcript import FRI_OPENINGS, poseidon_challenger
from zk_circuits import bitrev, blinding_counts, model_blinded_wires, model_salt

U64 = np.uint64
ORACLE_NAMES = ["constants || sigmas", "wires", "Z || partial products", "quotient chunks"]
ORACLE_BLINDING = [False, True, True, True]                         # PlonkOracle::{CONSTANTS_SIGMAS, WIRES, ZS_PARTIAL_PRODUCTS, QUOTIENT}.blinding (plonk_common.rs:23-46)
ZS_COLUMNS = ["Z of challenge 0", "Z of challenge 1"] + ["partial product %d of challenge %d" % (c, a) for a in range(2) for c in range(9)]


# ------------------------------------------------------------------------------- the two hashers
class PoseidonHashing:
    name, hasher = "poseidon", 0

    def __init__(self, orc):
        self.orc = orc

    def challenger(self):
        return poseidon_challenger(self.orc)

    def tree(self, leaves, cap_height):
        t = self.orc.merkle(np.ascontiguousarray(leaves, dtype=U64), cap_height)
        return SimpleNamespace(cap=t.cap, prove=t.prove, keep=t)

    def verify_path(self, leaf, index, cap, siblings):
        return fm.poseidon_verify_path(self.orc)(leaf, index, cap, siblings)

    def circuit_digest(self, cap, degree_bits):
        """circuit_builder.rs:1086-1098 with an empty domain separator: hash_no_pad(cap || hash_pad([]) || [degree_bits])"""
        empty = self.orc.hash_no_pad(np.array([1] + [0] * 10 + [1], dtype=U64))                     # hash_pad (config.rs:43-51), WIDTH = 12
        return self.orc.hash_no_pad(np.concatenate([np.asarray(cap, dtype=U64).reshape(-1), empty, np.array([degree_bits], dtype=U64)]))

    def pow_valid(self, state, pos, candidates, bits):
        states = np.tile(np.array(state, dtype=U64), (len(candidates), 1))
        states[:, pos] = candidates
        return self.orc.poseidon(states)[:, 7] >> U64(64 - bits) == 0


class KeccakHashing:
    name, hasher = "keccak", 1

    _permuted = {}                                                   # state -> KeccakPermutation of it: the cases replay one transcript many times

    def __init__(self, orc=None):
        import test_keccak
        self.k = test_keccak

    def challenger(self):
        from transcript import DuplexChallenger

        def permute(state):
            key = tuple(int(x) % P for x in state)
            if key not in self._permuted:
                self._permuted[key] = self.k.model_permute(key)
            return list(self._permuted[key])
        return DuplexChallenger(permute, self.k.model_hash_elements)

    def tree(self, leaves, cap_height):
        t = self.k.ModelTree(np.ascontiguousarray(leaves, dtype=U64))
        return SimpleNamespace(cap=t.cap(cap_height), prove=lambda i: t.prove(i, cap_height), keep=t)

    def verify_path(self, leaf, index, cap, siblings):
        return bool(self.k.model_verify_path(leaf, index, np.array(siblings, dtype=U64).reshape(-1, 4), cap))

    def circuit_digest(self, cap, degree_bits):
        return self.k.model_circuit_digest(cap, degree_bits)

    def pow_valid(self, state, pos, candidates, bits):
        return self.k.model_pow_responses(state, pos, np.asarray(candidates, dtype=U64)) >> U64(64 - bits) == 0


def hashing_of(orc, hasher):
    return KeccakHashing() if hasher in ("keccak", 1) else PoseidonHashing(orc)


# ------------------------------------------------------------------------------- the derivation
def _ext_words(vals):
    return np.array([w for v in vals for w in v], dtype=U64)


def quotient_points(lgN, count=64):
    """The fixed LDE points a sampled quotient comparison uses: the first, the last, one in each of the eight cosets of H (i = k mod 8), the
    rest spread evenly.  Every point of the coset evaluates every row's constraint polynomials, so no gate is left out by the choice."""
    N = 1 << lgN
    pts = {0, N - 1} | {(N // 8) * k + k for k in range(8)} | {(i * (N // count) + 3 * i) % N for i in range(count)}
    extra = 5
    while len(pts) < count:
        pts.add(extra * 2654435761 % N)
        extra += 1
    pts = sorted(pts)
    assert len(pts) >= count and {i % 8 for i in pts} == set(range(8))
    return pts


def quotient_at(d, cs_lde, wires_lde, zs_lde, pi_hash, betas, gammas, alphas, points):
    """{i: [vanishing_b(x_i) / Z_H(x_i) for the two challenges]} at the chosen LDE points (vanishing_model.vanishing_terms, reduced as
    vanishing_over_z_h reduces them)"""
    shape = vm.Shape(d)
    cs, wires, zs = vm._ints(cs_lde), vm._ints(wires_lde), vm._ints(zs_lde)
    out = {}
    for i in points:
        terms, z_h = vm.vanishing_terms(shape, i, cs, wires, zs, pi_hash, betas, gammas)
        z_h_inv = pow(z_h, P - 2, P)
        vals = []
        for b in range(2):
            acc = 0
            for t in reversed(terms):
                acc = (acc * alphas[b] + t) % P
            vals.append(acc * z_h_inv % P)
        out[i] = vals
    return out


def quotient_of_chunks_at(orc, chunks, lg, points):
    """{i: [t_b(x_i)]}: t_b(x) = sum_k chunk_{8 b + k}(x) x^(k n) at LDE point i, from the chunks' own LDE (prover.rs:245-258 backwards)"""
    n = 1 << lg
    lde = orc.lde(np.ascontiguousarray(chunks, dtype=U64), 3, threads=4)
    root = vm.primitive_root(lg + 3)
    out = {}
    for i in points:
        xn = pow(vm.COSET_SHIFT * pow(root, i, P) % P, n, P)
        vals = []
        for b in range(2):
            acc = 0
            for k in reversed(range(8)):
                acc = (acc * xn + int(lde[8 * b + k][i])) % P
            vals.append(acc)
        out[i] = vals
    return out


def derive(orc, hashing, d, constants_sigmas, wires, public_inputs, seed, quotient_chunks=None):
    """-> a namespace holding every part of the proof gl_prove_device_seeded(seed) has to give after gl_witness_blind(seed), and its bytes.
    `wires`: the UNBLINDED [135][n] witness.  `quotient_chunks`: None derives the 16 chunks from every LDE point; chunks handed in (the
    prover's own) are checked against the model at quotient_points() and then used as they are (m.quotient_sampled = True)."""
    assert d.zero_knowledge == 1 and d.num_lookup_polys == 0 and d.rate_bits == 3
    m = SimpleNamespace(times={}, hashing=hashing, d=d)
    t0 = time.perf_counter()

    def lap(name):
        nonlocal t0
        m.times[name] = time.perf_counter() - t0
        t0 = time.perf_counter()

    lg, rb, ch_ht, nc = d.degree_bits, d.rate_bits, d.cap_height, d.num_constants
    n, lgN = 1 << lg, lg + rb
    N = 1 << lgN
    g, q = d.num_gate_rows, d.num_query_rounds
    k_is = [int(d.k_is[j]) for j in range(NUM_SIGMAS)]
    cs_values = np.ascontiguousarray(constants_sigmas, dtype=U64)
    pis = np.asarray(public_inputs, dtype=U64)
    m.pi_hash = [int(x) for x in (orc.hash_no_pad(pis) if len(pis) else np.zeros(4, dtype=U64))]
    m.regular, m.pairs = blinding_counts(g, q)

    def commit(cols, from_values, oracle):
        """(coefficients, leaves in Merkle order with the salt behind them, their tree)"""
        ob = orc.batch(np.ascontiguousarray(cols, dtype=U64), rb, ch_ht, from_values=from_values, threads=4)
        leaves = ob.leaves()
        if ORACLE_BLINDING[oracle]:
            leaves = np.concatenate([leaves, model_salt(seed, oracle, lgN)], axis=1)
        return ob.polynomials, leaves, hashing.tree(leaves, ch_ht)

    # constants || sigmas, the circuit digest
    cs_coeffs, cs_leaves, cs_tree = commit(cs_values, True, 0)
    m.cs_cap = cs_tree.cap
    m.digest = hashing.circuit_digest(m.cs_cap, lg)
    # blind(), the wires oracle
    m.blinded = model_blinded_wires(np.asarray(wires, dtype=U64), g, seed, q)
    w_coeffs, w_leaves, w_tree = commit(m.blinded, True, 1)
    lap("wires")
    ch = hashing.challenger()
    ch.observe_hashes(m.digest)
    ch.observe_hashes(np.array(m.pi_hash, dtype=U64), inner=True)
    ch.observe_hashes(w_tree.cap)
    m.betas, m.gammas = ch.get(2), ch.get(2)
    # Z and the partial products
    zs = pm.partial_products(m.blinded[:NUM_SIGMAS], cs_values[nc:], k_is, m.betas, m.gammas, lg)
    m.zs = np.array(zs, dtype=U64)
    # every blinding row's sigma is the identity, so Z is back at 1 when the gate rows end and stays there through the last pair and the padding
    last = g + m.regular + 2 * m.pairs
    m.z_after_gate_rows = [int(m.zs[a][g]) for a in range(2)]
    m.z_after_pairs = [int(m.zs[a][last % n]) for a in range(2)]
    m.z_on_blinding_rows_is_one = bool((m.zs[:2, g:] == 1).all())
    z_coeffs, z_leaves, z_tree = commit(m.zs, True, 2)
    lap("Z and partial products")
    ch.observe_hashes(z_tree.cap)
    m.alphas = ch.get(2)
    # the quotient
    cs_lde, w_lde, z_lde = (orc.lde(c, rb, threads=4) for c in (cs_coeffs, w_coeffs, z_coeffs))
    m.quotient_sampled = quotient_chunks is not None
    if quotient_chunks is None:
        values = vm.vanishing_over_z_h(d, cs_lde, w_lde, z_lde, m.pi_hash, m.betas, m.gammas, m.alphas)
        coeffs = orc.coset_ifft(np.array(values, dtype=U64), vm.COSET_SHIFT)
        m.chunks = coeffs.reshape(2 * 8, n).copy()                  # trim_to_len(8 n), chunks(n) (prover.rs:245-258)
    else:
        m.chunks = np.ascontiguousarray(quotient_chunks, dtype=U64)
        m.points = quotient_points(lgN)
        m.quotient_model = quotient_at(d, cs_lde, w_lde, z_lde, m.pi_hash, m.betas, m.gammas, m.alphas, m.points)
        m.quotient_given = quotient_of_chunks_at(orc, m.chunks, lg, m.points)
    q_coeffs, q_leaves, q_tree = commit(m.chunks, False, 3)
    lap("quotient")
    ch.observe_hashes(q_tree.cap)
    m.caps = [w_tree.cap, z_tree.cap, q_tree.cap]
    m.zeta = ch.get(2)
    assert pow(m.zeta[0], n, P) != 1 or m.zeta[1]                    # "Opening point is in the subgroup" (prover.rs:280-283)
    # the openings
    root = vm.primitive_root(lg)
    gzeta = (m.zeta[0] * root % P, m.zeta[1] * root % P)
    groups = [cs_coeffs, w_coeffs, z_coeffs, q_coeffs]
    at_zeta = [[pm.eval_ext(col, m.zeta) for col in grp] for grp in groups]
    o = m.openings = {}
    o["constants"], o["sigmas"], o["wires"] = _ext_words(at_zeta[0][:nc]), _ext_words(at_zeta[0][nc:]), _ext_words(at_zeta[1])
    o["zs"], o["pp"], o["quotient"] = _ext_words(at_zeta[2][:NUM_ZS]), _ext_words(at_zeta[2][NUM_ZS:]), _ext_words(at_zeta[3])
    o["zs_next"] = _ext_words([pm.eval_ext(col, gzeta) for col in z_coeffs[:NUM_ZS]])
    o["lookups"] = o["lookups_next"] = np.zeros(0, dtype=U64)
    for name in FRI_OPENINGS:
        ch.observe(o[name])
    m.transcript_after_openings = (list(ch.state), list(ch.inp), list(ch.out))
    lap("openings")
    m.fri_alpha = ch.get(2)
    # FRI: combine and divide, commit phase (fri/prover.rs:69-112)
    coeffs = pm.combine_and_divide(groups, m.zeta, root, m.fri_alpha) + [(0, 0)] * (N - n)       # final_poly.lde(rate_bits)
    lap("combine and divide")
    shift = vm.COSET_SHIFT
    m.fri_caps, m.fri_betas, fri_leaves, fri_trees = [], [], [], []
    for r in range(d.num_fri_rounds):
        arity = 1 << d.fri_arity_bits[r]
        comps = orc.coset_fft(np.array([[c[0] for c in coeffs], [c[1] for c in coeffs]], dtype=U64), shift)
        values = np.stack([comps[0], comps[1]], axis=1)[bitrev(len(coeffs).bit_length() - 1)]      # reverse_index_bits_in_place
        leaves = values.reshape(len(coeffs) // arity, 2 * arity)      # flatten(chunk): each extension value's two words in order
        tree = hashing.tree(leaves, ch_ht)
        ch.observe_hashes(tree.cap)
        beta = ch.get(2)
        m.fri_caps.append(tree.cap); m.fri_betas.append(beta); fri_leaves.append(leaves); fri_trees.append(tree)
        coeffs = pm.fold(coeffs, arity, beta)
        shift = pow(shift, arity, P)
    assert all(c == (0, 0) for c in coeffs[len(coeffs) >> rb:])      # "The coefficients being removed here should always be zero."
    m.final_poly = _ext_words(coeffs[:len(coeffs) >> rb])
    ch.observe(m.final_poly)
    lap("commit phase")
    # proof of work (fri/prover.rs:114-160): the smallest witness, scanned from 0
    state = list(ch.state)
    state[:len(ch.inp)] = ch.inp
    m.pow_witness, base = None, 0
    while m.pow_witness is None:
        cand = np.arange(base, base + 4096, dtype=U64)
        ok = np.flatnonzero(hashing.pow_valid(state, len(ch.inp), cand, d.proof_of_work_bits))
        if len(ok):
            m.pow_witness = int(cand[ok[0]])
        base += 4096
    ch.observe([m.pow_witness])
    m.pow_response = ch.get(1)[0]
    assert m.pow_response >> (64 - d.proof_of_work_bits) == 0
    lap("proof of work")
    # the query rounds (fri/prover.rs:162-216)
    m.x_index = [ch.get(1)[0] % N for _ in range(q)]
    initial = [(cs_leaves, cs_tree), (w_leaves, w_tree), (z_leaves, z_tree), (q_leaves, q_tree)]
    m.queries = []
    for x in m.x_index:
        init = [(leaves[x].copy(), tree.prove(x)) for leaves, tree in initial]
        steps = []
        for r in range(d.num_fri_rounds):
            x >>= d.fri_arity_bits[r]
            steps.append((fri_leaves[r][x].copy(), fri_trees[r].prove(x)))
        m.queries.append((init, steps))
    m.leaves = [cs_leaves, w_leaves, z_leaves, q_leaves]
    m.bytes = proof_bytes(d, m.caps, m.openings, m.fri_caps, m.queries, m.final_poly, m.pow_witness, pis)
    lap("queries")
    return m


# ------------------------------------------------------------------------------- naming the first difference
def describe_difference(d, got_bytes, m):
    """None if `got_bytes` are the model's, else the first section of the proof that differs, by name"""
    if bytes(got_bytes) == m.bytes:
        return None
    if len(got_bytes) != len(m.bytes):
        return "the proof has %d bytes, the model's %d" % (len(got_bytes), len(m.bytes))
    pp = ParsedProof(d, bytes(got_bytes))

    def words(name, got, want):
        got, want = np.asarray(got, dtype=U64).reshape(-1), np.asarray(want, dtype=U64).reshape(-1)
        bad = np.flatnonzero(got != want)
        if len(bad):
            return "%s: %d of %d words differ, first word %d: got %d, model %d" % (name, len(bad), want.size, bad[0], got[bad[0]], want[bad[0]])

    def hashes(name, got, want, unit):
        got, want = np.asarray(got, dtype=U64).reshape(-1, 4), np.asarray(want, dtype=U64).reshape(-1, 4)
        bad = np.flatnonzero((got != want).any(axis=1))
        if len(bad):
            return "%s: %d of %d hashes differ, first %s %d" % (name, len(bad), len(want), unit, bad[0])

    for k, name in enumerate(ORACLE_NAMES[1:]):
        why = hashes("cap of the %s oracle" % name, pp.caps[k], m.caps[k], "cap entry")
        if why:
            return why
    for name, count in opening_columns(d):
        got, want = np.asarray(pp.openings[name]).reshape(-1, 2), np.asarray(m.openings[name]).reshape(-1, 2)
        bad = np.flatnonzero((got != want).any(axis=1))
        if len(bad):
            return "openings '%s': %d of %d columns differ, first column %d: got %s, model %s" % (name, len(bad), count, bad[0], got[bad[0]], want[bad[0]])
    for r in range(d.num_fri_rounds):
        why = hashes("FRI commit cap of round %d" % r, pp.fri_caps[r], m.fri_caps[r], "cap entry")
        if why:
            return why
    got, want = pp.final_poly.reshape(-1, 2), m.final_poly.reshape(-1, 2)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        return "final polynomial: %d of %d coefficients differ, first coefficient %d: got %s, model %s" % (len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])
    if pp.pow_witness != m.pow_witness:
        return "PoW witness: got %d, the smallest is %d" % (pp.pow_witness, m.pow_witness)
    for qi, ((init, steps), (minit, msteps)) in enumerate(zip(pp.queries, m.queries)):
        trees = [("initial tree of the %s oracle" % ORACLE_NAMES[o], init[o], minit[o]) for o in range(4)]
        trees += [("FRI tree of round %d" % r, steps[r], msteps[r]) for r in range(d.num_fri_rounds)]
        for name, (leaf, sibs), (mleaf, msibs) in trees:
            where = "query %d (index %d), %s" % (qi, m.x_index[qi], name)
            why = words(where + ", leaf", leaf, mleaf) or hashes(where + ", path", sibs, msibs, "sibling level")
            if why:
                return why
    if not (pp.public_inputs == np.asarray(ParsedProof(d, m.bytes).public_inputs)).all():
        return "public inputs differ"
    return "the bytes differ where the parser reads nothing: padding of a hash"


def columns_difference(name, columns, got, want):
    """None, or the first column of a captured intermediate that differs from the model's"""
    got, want = np.asarray(got, dtype=U64), np.asarray(want, dtype=U64)
    if got.shape != want.shape:
        return "%s: shape %s, the model's %s" % (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        c, r = (int(v) for v in bad[0])
        return "%s: %d of %d words differ, first: %s, row %d: got %d, model %d" % (name, len(bad), want.size, columns[c], r, got[c, r], want[c, r])


# ------------------------------------------------------------------------------- the verifier
class E:
    """an element of F_p^2 = F_p[X] / (X^2 - 7) with the operators vanishing_model's gate functions use, so that they evaluate a gate's
    constraints on extension-field values (EvaluationVars) unchanged; `% P` is the identity"""
    __slots__ = ("a", "b")

    def __init__(self, a, b=0):
        self.a, self.b = a % P, b % P

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(int(x))

    def __add__(self, o):
        o = E.of(o)
        return E(self.a + o.a, self.b + o.b)

    __radd__ = __add__

    def __sub__(self, o):
        o = E.of(o)
        return E(self.a - o.a, self.b - o.b)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        return E(self.a * o.a + vm.W * self.b * o.b, self.a * o.b + self.b * o.a)

    __rmul__ = __mul__

    def __lshift__(self, k):
        return self * (1 << k)

    def __mod__(self, p):
        assert p == P
        return self

    def __pow__(self, e, mod=None):
        r, base = E(1), self
        while e:
            if e & 1:
                r = r * base
            base = base * base
            e >>= 1
        return r

    def __eq__(self, o):
        o = E.of(o)
        return (self.a, self.b) == (o.a, o.b)

    def inv(self):
        t = fm._ext_inv((self.a, self.b))
        return E(t[0], t[1])


def vanishing_identity_holds(d, pp, pi_hash, betas, gammas, alphas, zeta):
    """plonk/verifier.rs:49-96 for a circuit without lookups: eval_vanishing_poly (vanishing_poly.rs:54-161) at zeta from the opening set,
    against Z_H(zeta) reduce_with_powers(quotient chunk openings, zeta^n)"""
    shape = vm.Shape(d)
    n = 1 << d.degree_bits
    ext = lambda name: [E(int(a), int(b)) for a, b in np.asarray(pp.openings[name], dtype=U64).reshape(-1, 2)]      # noqa: E731
    consts, sigmas, w, zs, zs_next, pps, quot = (ext(k) for k in ("constants", "sigmas", "wires", "zs", "zs_next", "pp", "quotient"))
    x = E(zeta[0], zeta[1])
    x_n = x ** n
    z_h = x_n - 1
    l_0 = z_h * ((x - 1) * n).inv()                                  # eval_l_0 (plonk_common.rs:57-71)
    terms = [l_0 * (zs[a] - 1) for a in range(2)]
    for a in range(2):
        accs = [zs[a]] + pps[9 * a:9 * a + 9] + [zs_next[a]]
        for c in range(vm.NUM_CHUNKS):
            num = den = E(1)
            for j in range(vm.CHUNK * c, vm.CHUNK * (c + 1)):
                num = num * (w[j] + x * (shape.k_is[j] * betas[a] % P) + gammas[a])
                den = den * (w[j] + sigmas[j] * betas[a] + gammas[a])
            terms.append(accs[c] * num - accs[c + 1] * den)
    gate_consts = consts[shape.num_selectors + shape.num_lookup_selectors:]
    by_index = []
    for gi, (constraints, selector_index, group_start, group_end) in enumerate(shape.gates):
        f = vm.gate_filter(gi, group_start, group_end, consts[selector_index], shape.num_selectors > 1)
        cons = constraints(gate_consts, w, pi_hash)
        by_index += [E(0)] * (len(cons) - len(by_index))
        for j, v in enumerate(cons):
            by_index[j] = by_index[j] + E.of(f) * E.of(v)
    terms += by_index
    for b in range(2):
        acc = E(0)
        for t in reversed(terms):
            acc = acc * alphas[b] + t
        t_zeta = E(0)
        for c in reversed(quot[8 * b:8 * b + 8]):
            t_zeta = t_zeta * x_n + c
        if not acc == z_h * t_zeta:
            return False
    return True


def fri_instance(d, zeta):
    """get_fri_instance (circuit_data.rs:564-597) with the blinded oracles marked: what fri_openings_model.verify reads"""
    ncs = d.num_constants + NUM_SIGMAS
    root = vm.primitive_root(d.degree_bits)
    names = [[(o, c) for c in range(w)] for o, w in enumerate((ncs, NUM_WIRES, NUM_ZS_PP, NUM_QUOTIENT))]
    at_zeta, at_gzeta = pm.opened_polys(names)
    zeta = (int(zeta[0]) % P, int(zeta[1]) % P)
    return SimpleNamespace(oracles=list(zip((ncs, NUM_WIRES, NUM_ZS_PP, NUM_QUOTIENT), ORACLE_BLINDING)),
                           batches=[(zeta, at_zeta), ((zeta[0] * root % P, zeta[1] * root % P), at_gzeta)])


def fri_params(d):
    return SimpleNamespace(degree_bits=d.degree_bits, rate_bits=d.rate_bits, cap_height=d.cap_height, proof_of_work_bits=d.proof_of_work_bits,
                           num_query_rounds=d.num_query_rounds, reduction_arity_bits=[d.fri_arity_bits[r] for r in range(d.num_fri_rounds)],
                           hiding=bool(d.zero_knowledge), hasher=d.hasher)


def fri_part(d, by, num_public_inputs):
    """the FriProof inside a proof's bytes: from the commit-phase caps to the PoW witness"""
    start = 3 * (1 << d.cap_height) * hash_bytes(d) + 16 * sum(k for _, k in opening_columns(d))
    return start, len(by) - 8 - 8 * num_public_inputs


def verify(orc, hashing, d, cs_cap, digest, by, public_inputs=None, trace=None):
    """-> the GL_CHECK_* code of the first failing check of VerifierCircuitData::verify (0: accepted) on a zero-knowledge proof's bytes:
    the vanishing identity, then verify_fri_proof.  Shape faults answer as fri_openings_model's parser names them."""
    try:
        pp = ParsedProof(d, bytes(by))
    except (AssertionError, ValueError, IndexError):
        return fm.LENGTH
    if public_inputs is not None and len(pp.public_inputs) != len(public_inputs):
        return fm.PUBLIC_INPUT_COUNT
    pis = pp.public_inputs
    pi_hash = [int(x) for x in (orc.hash_no_pad(pis % U64(P)) if len(pis) else np.zeros(4, dtype=U64))]
    ch = hashing.challenger()
    ch.observe_hashes(digest)
    ch.observe_hashes(np.array(pi_hash, dtype=U64), inner=True)
    ch.observe_hashes(pp.caps[0])
    betas, gammas = ch.get(2), ch.get(2)
    ch.observe_hashes(pp.caps[1])
    alphas = ch.get(2)
    ch.observe_hashes(pp.caps[2])
    zeta = ch.get(2)
    for name in FRI_OPENINGS:
        ch.observe(pp.openings[name])
    if trace is not None:
        trace.update(betas=betas, gammas=gammas, alphas=alphas, zeta=zeta, parsed=pp)
    if not vanishing_identity_holds(d, pp, pi_hash, betas, gammas, alphas, zeta):
        return fm.VANISHING
    openings = np.concatenate([np.asarray(pp.openings[name], dtype=U64) for name in FRI_OPENINGS]).reshape(-1, 2)
    caps = np.array([np.asarray(cs_cap, dtype=U64).reshape(-1, 4)] + [np.asarray(c, dtype=U64) for c in pp.caps], dtype=U64)
    start, end = fri_part(d, by, len(pis))
    return fm.verify(fri_params(d), fri_instance(d, zeta), caps, openings, ch, bytes(by)[start:end], hashing.verify_path, trace=trace)


# ------------------------------------------------------------------------------- byte offsets, for the tamper tests
def layout(d, num_public_inputs):
    """Byte offsets inside ProofWithPublicInputs::to_bytes of a zero-knowledge proof: caps[k], openings[name], fri_caps[r], per query round
    q leaf[q][o] / sibling[q][o] of the four initial trees and step_evals[q][r] / step_sibling[q][r], final, pow, end."""
    from proof_parser import leaf_lens
    hb, ncap, lgN = hash_bytes(d), 1 << d.cap_height, d.degree_bits + d.rate_bits
    lay = SimpleNamespace(caps=[k * ncap * hb for k in range(3)], openings={}, fri_caps=[], leaf=[], sibling=[], step_evals=[], step_sibling=[],
                          leaf_len=leaf_lens(d))
    at = 3 * ncap * hb
    for name, k in opening_columns(d):
        lay.openings[name] = at
        at += 16 * k
    for r in range(d.num_fri_rounds):
        lay.fri_caps.append(at)
        at += ncap * hb
    for _ in range(d.num_query_rounds):
        leaf, sibling, step_evals, step_sibling, lg = [], [], [], [], lgN
        for k in lay.leaf_len:
            leaf.append(at)
            sibling.append(at + 8 * k + 1)
            at += 8 * k + 1 + (lgN - d.cap_height) * hb
        for r in range(d.num_fri_rounds):
            lg -= d.fri_arity_bits[r]
            step_evals.append(at)
            step_sibling.append(at + 8 * (2 << d.fri_arity_bits[r]) + 1)
            at += 8 * (2 << d.fri_arity_bits[r]) + 1 + (lg - d.cap_height) * hb
        lay.leaf.append(leaf); lay.sibling.append(sibling); lay.step_evals.append(step_evals); lay.step_sibling.append(step_sibling)
    lay.final = at
    lay.pow = at + 16 * ((1 << d.degree_bits) >> sum(d.fri_arity_bits[r] for r in range(d.num_fri_rounds)))
    lay.end = lay.pow + 8 + 8 + 8 * num_public_inputs
    return lay


def flip(by, offset, bit=0):
    b = bytearray(by)
    b[offset] ^= 1 << bit
    return bytes(b)
