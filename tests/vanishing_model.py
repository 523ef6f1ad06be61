"""A plain Python-integer model of vanishing(x) / Z_H(x) on the LDE coset (no tests here).

What the prover's quotient launches (csrc/prover_kernels.cuh: k_quotient<false / true>, k_quotient_lookup, k_quotient_random_access,
k_quotient_ext_arith) compute per point x_i = 7 w_N^i, written from the reference, in the reference's term order:
  plonk/vanishing_poly.rs:164-325   eval_vanishing_poly_base_batch: L_0(x)(Z(x) - 1), the partial-product checks, the lookup terms,
                                    the gate terms; one alpha-weighted sum per challenge (plonk_common.rs:97-114)
  plonk/vanishing_poly.rs:510-668   check_lookup_constraints_batch, :31-49 get_lut_poly
  util/partial_products.rs:52-76    check_partial_products
  plonk/plonk_common.rs:57-71, field/src/zero_poly_coset.rs:55-60   L_0(x) = Z_H(x) / (n (x - 1)), Z_H(x) = x^n - 1
  gates/gate.rs:121-146,277-284     the filter, the constants behind the selector prefix; vanishing_poly.rs:706-732: constraint j of
                                    every gate is added into term j
  gates/*.rs                        each gate's eval_unfiltered (cited at the function)
Only Python `int` arithmetic mod P: no numpy on field values, no oracle, no product library.  Every argument may be non-satisfying: the
result is then simply not a polynomial multiple of Z_H, but still the value the kernels have to produce.
"""
import os
import sys

P = 2**64 - 2**32 + 1
W = 7                                   # Extendable<2>::W (field/src/goldilocks_extensions.rs:19)
COSET_SHIFT = 7                         # F::coset_shift() = MULTIPLICATIVE_GROUP_GENERATOR (field/src/types.rs:437, goldilocks_field.rs:80)
UNUSED_SELECTOR = 2**32 - 1             # gates/selectors.rs:14
NUM_WIRES, NUM_ROUTED, CHUNK, NUM_CHUNKS = 135, 80, 8, 10

# gl_circuit_desc gate codes (include/plonky2_mi355x.h)
(NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC, POSEIDON, BASE_SUM, LOOKUP, LOOKUP_TABLE, EXPONENTIATION, RANDOM_ACCESS, ARITHMETIC_EXT, MUL_EXT,
 REDUCING, REDUCING_EXT) = range(14)
LOOKUP_SLOTS, LOOKUP_TABLE_SLOTS = 40, 26       # gates/lookup.rs:44-47 (80 / 2), gates/lookup_table.rs:49-52 (80 / 3)
# lookup selectors (gates/selectors.rs:34-40) and lookup challenges (plonk/circuit_builder.rs:66-71)
TRANS_SRE, TRANS_LDC, INIT_SRE, LAST_LDC, START_END = range(5)
CH_A, CH_B, CH_ALPHA, CH_DELTA = range(4)


def primitive_root(lg):
    """F::primitive_root_of_unity(lg): POWER_OF_TWO_GENERATOR = 7^((P - 1) / 2^32) squared 32 - lg times (field/src/types.rs, primitive_root_of_unity)"""
    return pow(7, (P - 1) >> lg, P)


assert primitive_root(32) == 1753635133440165772      # POWER_OF_TWO_GENERATOR (field/src/goldilocks_field.rs:87)


# ------------------------------------------------------------------------------- F_p^2 = F_p[X] / (X^2 - 7)
def _ext_mul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


# ------------------------------------------------------------------------------- Poseidon (hash/poseidon.rs), textbook rounds
_POSEIDON = None


def _poseidon_tables():
    """the committed round constants (tools/poseidon_round_constants.txt) and the MDS matrix, as tests/golden/make_golden.py reads them"""
    global _POSEIDON
    if _POSEIDON is None:
        tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
        if tools not in sys.path:
            sys.path.insert(0, tools)
        import gen_poseidon_constants as g
        _POSEIDON = (g.load_round_constants(), g.mds_matrix())
    return _POSEIDON


def _mds(M, s):
    return [sum(a * b for a, b in zip(row, s)) % P for row in M]


# ------------------------------------------------------------------------------- the gates: (constants, wires, pi_hash) -> constraints
def _constant_gate(c, w, pi):
    """ConstantGate { num_consts: 2 } (gates/constant.rs:58-73)"""
    return [(c[i] - w[i]) % P for i in range(2)]


def _public_input_gate(c, w, pi):
    """PublicInputGate (gates/public_input.rs:42-58): wires 0..4 against the public-inputs hash"""
    return [(w[i] - pi[i]) % P for i in range(4)]


def _arithmetic_gate(c, w, pi):
    """ArithmeticGate { num_ops: 20 } (gates/arithmetic_base.rs:44-55,72-103): output - (m0 m1 c0 + addend c1)"""
    return [(w[4 * i + 3] - (w[4 * i] * w[4 * i + 1] * c[0] + w[4 * i + 2] * c[1])) % P for i in range(20)]


# PoseidonGate wire columns (gates/poseidon.rs:36-95): inputs 0..11, outputs 12..23, the swap bit, the four deltas, then the S-box INPUTS of
# the first full rounds 1..3 (round 0 reads the inputs), of the 22 partial rounds (word 0) and of the four last full rounds
PSD_WIRE_SWAP, PSD_WIRE_DELTA = 24, 25
PSD_WIRE_FULL0_SBOX, PSD_WIRE_PARTIAL_SBOX, PSD_WIRE_FULL1_SBOX = 29, 65, 87
PSD_FULL_SBOX_WIRES = list(range(PSD_WIRE_FULL0_SBOX, PSD_WIRE_FULL0_SBOX + 36)) + list(range(PSD_WIRE_FULL1_SBOX, PSD_WIRE_FULL1_SBOX + 48))
PSD_PARTIAL_SBOX_WIRES = list(range(PSD_WIRE_PARTIAL_SBOX, PSD_WIRE_PARTIAL_SBOX + 22))


def _poseidon_gate(c, w, pi):
    """PoseidonGate (gates/poseidon.rs:36-95 the wires, :193-272 the constraints).  The reference evaluates the partial rounds in their
    factorised form (partial_first_constant_layer, mds_partial_layer_init / _fast); the factorisation is linear algebra on the round
    constants and the MDS matrix that treats every S-box OUTPUT as a free variable and keeps state[0] at every S-box input, so the
    textbook rounds below give the same constraints whatever the S-box input wires hold."""
    rc, M = _poseidon_tables()
    swap = w[PSD_WIRE_SWAP]
    out = [swap * (swap - 1) % P]
    s = list(w[0:12])
    for i in range(4):
        delta = w[PSD_WIRE_DELTA + i]
        out.append((swap * (w[i + 4] - w[i]) - delta) % P)
        s[i], s[i + 4] = (w[i] + delta) % P, (w[i + 4] - delta) % P
    r = 0
    for k in range(4):                                  # first full rounds; the S-box inputs of round 0 are not wires
        s = [(a + b) % P for a, b in zip(s, rc[r])]
        if k:
            sbox_in = w[PSD_WIRE_FULL0_SBOX + 12 * (k - 1):PSD_WIRE_FULL0_SBOX + 12 * k]
            out += [(a - b) % P for a, b in zip(s, sbox_in)]
            s = list(sbox_in)
        s = _mds(M, [pow(a, 7, P) for a in s]); r += 1
    for k in range(22):                                 # partial rounds
        s = [(a + b) % P for a, b in zip(s, rc[r])]
        out.append((s[0] - w[PSD_WIRE_PARTIAL_SBOX + k]) % P)
        s[0] = pow(w[PSD_WIRE_PARTIAL_SBOX + k], 7, P)
        s = _mds(M, s); r += 1
    for k in range(4):                                  # second full rounds
        s = [(a + b) % P for a, b in zip(s, rc[r])]
        sbox_in = w[PSD_WIRE_FULL1_SBOX + 12 * k:PSD_WIRE_FULL1_SBOX + 12 * (k + 1)]
        out += [(a - b) % P for a, b in zip(s, sbox_in)]
        s = _mds(M, [pow(a, 7, P) for a in sbox_in]); r += 1
    return out + [(s[i] - w[12 + i]) % P for i in range(12)]


def _base_sum_gate(c, w, pi):
    """BaseSumGate<2> { num_limbs: 63 } (gates/base_sum.rs:38-50,67-80): wire 0 the sum, wires 1..=63 the limbs, little-endian
    (reduce_with_powers, plonk_common.rs:116-128); then limb (limb - 1) per limb"""
    limbs = w[1:64]
    return [(sum(l << i for i, l in enumerate(limbs)) - w[0]) % P] + [l * (l - 1) % P for l in limbs]


def _exponentiation_gate(c, w, pi):
    """ExponentiationGate { num_power_bits: 66 } (gates/exponentiation.rs:47-71,88-121): wire 0 base, 1..=66 the bits little-endian,
    67 output, 68..134 the intermediate values; accumulated from the top bit"""
    nb = 66
    base, bits, output, inter = w[0], w[1:1 + nb], w[1 + nb], w[2 + nb:2 + 2 * nb]
    out = []
    for i in range(nb):
        prev = 1 if i == 0 else inter[i - 1] * inter[i - 1]
        bit = bits[nb - 1 - i]
        out.append((prev * (bit * base + 1 - bit) - inter[i]) % P)
    return out + [(output - inter[nb - 1]) % P]


def random_access_layout(bits):
    """RandomAccessGate::new_from_config (gates/random_access.rs:55-71): (num_copies, num_extra_constants)"""
    vec = 1 << bits
    copies = min(NUM_ROUTED // (2 + vec), NUM_WIRES // (2 + vec + bits))
    return copies, min(NUM_ROUTED - (2 + vec) * copies, 2)


def _random_access_gate(bits):
    """RandomAccessGate (gates/random_access.rs:79-117 the wires, :139-184 the constraints)"""
    vec = 1 << bits
    copies, extra = random_access_layout(bits)
    routed = (2 + vec) * copies + extra

    def gate(c, w, pi):
        out = []
        for k in range(copies):
            at = (2 + vec) * k
            index, claimed, items = w[at], w[at + 1], list(w[at + 2:at + 2 + vec])
            b = [w[routed + k * bits + i] for i in range(bits)]
            out += [x * (x - 1) % P for x in b]
            rec = 0
            for x in reversed(b):
                rec = 2 * rec + x
            out.append((rec - index) % P)
            for x in b:
                items = [(items[2 * j] + x * (items[2 * j + 1] - items[2 * j])) % P for j in range(len(items) // 2)]
            out.append((items[0] - claimed) % P)
        return out + [(c[i] - w[(2 + vec) * copies + i]) % P for i in range(extra)]
    return gate


def _arithmetic_ext_gate(c, w, pi):
    """ArithmeticExtensionGate { num_ops: 10 } (gates/arithmetic_extension.rs:40-51,87-105): output - (c0 m0 m1 + c1 addend)"""
    out = []
    for i in range(10):
        m0, m1, ad, o = ((w[8 * i + 2 * k], w[8 * i + 2 * k + 1]) for k in range(4))
        pr = _ext_mul(m0, m1)
        out += [(o[k] - (pr[k] * c[0] + ad[k] * c[1])) % P for k in range(2)]
    return out


def _mul_ext_gate(c, w, pi):
    """MulExtensionGate { num_ops: 13 } (gates/multiplication_extension.rs:65-96): output - c0 m0 m1"""
    out = []
    for i in range(13):
        m0, m1, o = ((w[6 * i + 2 * k], w[6 * i + 2 * k + 1]) for k in range(3))
        pr = _ext_mul(m0, m1)
        out += [(o[k] - pr[k] * c[0]) % P for k in range(2)]
    return out


def _reducing_gate(ext):
    """ReducingGate { num_coeffs: 43 } (gates/reducing.rs:29-55,100-120; base-field coefficients) and ReducingExtensionGate
    { num_coeffs: 32 } (gates/reducing_extension.rs:29-58,102-121): wires 0-1 output, 2-3 alpha, 4-5 old_acc, the coefficients, the
    accumulators; the last accumulator is the output.  acc alpha + coeff_i - acc_i"""
    nc, width = (32, 2) if ext else (43, 1)
    acc0 = 6 + width * nc

    def gate(c, w, pi):
        alpha, acc, out = (w[2], w[3]), (w[4], w[5]), []
        for i in range(nc):
            at = 0 if i == nc - 1 else acc0 + 2 * i
            co = (w[6 + 2 * i], w[6 + 2 * i + 1]) if ext else (w[6 + i], 0)
            pr = _ext_mul(acc, alpha)
            out += [(pr[k] + co[k] - w[at + k]) % P for k in range(2)]
            acc = (w[at], w[at + 1])
        return out
    return gate


_NO_CONSTRAINTS = lambda c, w, pi: []
_GATES = {NOOP: _NO_CONSTRAINTS, LOOKUP: _NO_CONSTRAINTS, LOOKUP_TABLE: _NO_CONSTRAINTS, CONSTANT: _constant_gate,
          PUBLIC_INPUT: _public_input_gate, ARITHMETIC: _arithmetic_gate, POSEIDON: _poseidon_gate, BASE_SUM: _base_sum_gate,
          EXPONENTIATION: _exponentiation_gate, ARITHMETIC_EXT: _arithmetic_ext_gate, MUL_EXT: _mul_ext_gate,
          REDUCING: _reducing_gate(False), REDUCING_EXT: _reducing_gate(True)}
_GATES.update({(RANDOM_ACCESS, bits): _random_access_gate(bits) for bits in range(1, 7)})


def gate_constraints(gate_type, param=0):
    """the function (constants behind the selector prefix, 135 wires, public-inputs hash) -> the gate's constraints.  NoopGate
    (gates/noop.rs), LookupGate (gates/lookup.rs:78-92) and LookupTableGate (gates/lookup_table.rs:93-107) have none."""
    return _GATES[(RANDOM_ACCESS, param)] if gate_type == RANDOM_ACCESS else _GATES[gate_type]


def gate_filter(g, group_start, group_end, sel, many_selectors):
    """compute_filter (gates/gate.rs:277-284): non-zero where the selector column holds this gate's index"""
    f = 1
    for k in list(range(group_start, group_end)) + ([UNUSED_SELECTOR] if many_selectors else []):
        if k != g:
            f = f * (k - sel) % P
    return f


# ------------------------------------------------------------------------------- the lookup argument
def lut_poly_at_delta(table, b, delta):
    """get_lut_poly(..).eval(delta) (vanishing_poly.rs:31-49,576-586): the table's combos inp + b out, zero-padded to whole
    LookupTableGate rows, then REVERSED into coefficients: combo_i is the coefficient of delta^(degree - 1 - i)"""
    degree = LOOKUP_TABLE_SLOTS * -(-len(table) // LOOKUP_TABLE_SLOTS)
    return sum((inp + b * out) * pow(delta, degree - 1 - i, P) for i, (inp, out) in enumerate(table)) % P


def _lookup_terms(tables, w, sel, lz, lz_next, d):
    """check_lookup_constraints_batch (vanishing_poly.rs:510-668) for one challenge: `sel` the lookup selectors, `lz` / `lz_next` the
    num_lookup_polys lookup polynomials here and at g x, `d` the four lookup challenges"""
    num_sldc = len(lz) - 1
    lu_degree, lut_degree = 8 - 1, -(-LOOKUP_TABLE_SLOTS // num_sldc)
    z_re, sldc, sldc_next = lz[0], lz[1:], lz_next[1:]
    looked = [(w[3 * s] + d[CH_A] * w[3 * s + 1]) % P for s in range(LOOKUP_TABLE_SLOTS)]        # lookup_table.rs:55-67
    looking = [(w[2 * s] + d[CH_A] * w[2 * s + 1]) % P for s in range(LOOKUP_SLOTS)]              # lookup.rs:49-56
    combos = [(w[3 * s] + d[CH_B] * w[3 * s + 1]) % P for s in range(LOOKUP_TABLE_SLOTS)]
    out = [sel[LAST_LDC] * sldc[num_sldc - 1] % P, sel[INIT_SRE] * sldc[0] % P, sel[INIT_SRE] * z_re % P]
    for t, table in enumerate(tables):
        out.append(sel[START_END + t] * (z_re - lut_poly_at_delta(table, d[CH_B], d[CH_DELTA])) % P)
    cur = lz_next[0]
    for e in combos:
        cur = (cur * d[CH_DELTA] + e) % P
    out.append(sel[TRANS_SRE] * (z_re - cur) % P)
    for poly in range(num_sldc):
        lut_f = [(d[CH_ALPHA] - looked[i]) % P for i in range(poly * lut_degree, min((poly + 1) * lut_degree, LOOKUP_TABLE_SLOTS))]
        lu_f = [(d[CH_ALPHA] - looking[i]) % P for i in range(poly * lu_degree, min((poly + 1) * lu_degree, LOOKUP_SLOTS))]

        def prod(fs, skip=None):
            r = 1
            for j, f in enumerate(fs):
                if j != skip:
                    r = r * f % P
            return r
        lu_sum = sum(prod(lu_f, i) for i in range(len(lu_f)))
        lut_sum_mul = sum(w[3 * (poly * lut_degree + i) + 2] * prod(lut_f, i) for i in range(len(lut_f)))
        prev = sldc_next[num_sldc - 1] if poly == 0 else sldc[poly - 1]
        out.append(sel[TRANS_SRE] * (prod(lut_f) * (sldc[poly] - prev) - lut_sum_mul) % P)
        out.append(sel[TRANS_LDC] * (prod(lu_f) * (sldc[poly] - prev) + lu_sum) % P)
    return out


# ------------------------------------------------------------------------------- the whole vanishing polynomial
def _ints(a):
    return [[int(v) for v in (col.tolist() if hasattr(col, "tolist") else col)] for col in a]


class Shape:
    """what the model reads of a circuit description (gl_circuit_desc), as plain Python values"""

    def __init__(self, d):
        self.degree_bits, self.num_constants, self.num_selectors = d.degree_bits, d.num_constants, d.num_selectors
        self.num_lookup_selectors, self.num_lookup_polys = d.num_lookup_selectors, d.num_lookup_polys
        self.k_is = [int(d.k_is[j]) for j in range(NUM_ROUTED)]
        self.gates = [(gate_constraints(d.gate_types[g], d.gate_params[g]), d.gate_selector_index[g], d.gate_group_start[g], d.gate_group_end[g])
                      for g in range(d.num_gates)]
        self.tables = [[(int(a), int(b)) for a, b in d.lookup_table(t)] for t in range(d.num_luts)]
        self.term0 = 2 + 2 * NUM_CHUNKS + (2 * (4 + d.num_luts + 2 * (d.num_lookup_polys - 1)) if d.num_lookup_polys else 0)


def vanishing_terms(shape, i, cs, wires, zs, pi_hash, betas, gammas, deltas=None):
    """(every term of the vanishing polynomial at LDE point i in the reference's order (vanishing_poly.rs:312-316), Z_H(x_i)); all
    arguments Python integers, the LDE arrays [column][N]; the gate terms start at shape.term0"""
    d = shape
    n, N = 1 << d.degree_bits, 1 << (d.degree_bits + 3)
    x = COSET_SHIFT * pow(primitive_root(d.degree_bits + 3), i, P) % P
    i_next = (i + 8) % N                                # g x = w_n x = w_N^8 x
    consts = [col[i] for col in cs[:d.num_constants]]
    sigmas = [col[i] for col in cs[d.num_constants:d.num_constants + NUM_ROUTED]]
    w = [col[i] for col in wires]
    z_h = (pow(x, n, P) - 1) % P
    l_0 = z_h * pow(n * (x - 1) % P, P - 2, P) % P
    terms = [l_0 * (zs[a][i] - 1) % P for a in range(2)]
    for a in range(2):
        accs = [zs[a][i]] + [zs[2 + 9 * a + c][i] for c in range(NUM_CHUNKS - 1)] + [zs[a][i_next]]
        for c in range(NUM_CHUNKS):
            num = den = 1
            for j in range(CHUNK * c, CHUNK * (c + 1)):
                num = num * (w[j] + betas[a] * (d.k_is[j] * x % P) + gammas[a]) % P
                den = den * (w[j] + betas[a] * sigmas[j] + gammas[a]) % P
            terms.append((accs[c] * num - accs[c + 1] * den) % P)
    nlp = d.num_lookup_polys
    if nlp:
        lookup_sel = consts[d.num_selectors:d.num_selectors + d.num_lookup_selectors]
        for a in range(2):
            lz = [zs[20 + nlp * a + k][i] for k in range(nlp)]
            lz_next = [zs[20 + nlp * a + k][i_next] for k in range(nlp)]
            terms += _lookup_terms(d.tables, w, lookup_sel, lz, lz_next, deltas[4 * a:4 * a + 4])
    assert len(terms) == d.term0
    gate_consts = consts[d.num_selectors + d.num_lookup_selectors:]
    by_index = []
    for g, (constraints, selector_index, group_start, group_end) in enumerate(d.gates):
        f = gate_filter(g, group_start, group_end, consts[selector_index], d.num_selectors > 1)
        cons = constraints(gate_consts, w, pi_hash)
        by_index += [0] * (len(cons) - len(by_index))
        for j, v in enumerate(cons):
            by_index[j] = (by_index[j] + f * v) % P
    return terms + by_index, z_h


def vanishing_over_z_h(desc, cs_lde, wires_lde, zs_lde, pi_hash, betas, gammas, alphas, deltas=None):
    """-> [2][N]: sum_t alpha_b^t term_t(x_i) / Z_H(x_i) at every LDE point, what coset_ifft turns into the quotient chunks
    (plonk/prover.rs:576-737).  `deltas` (8 values) for circuits with lookups."""
    shape = Shape(desc)
    cs, wires, zs = _ints(cs_lde), _ints(wires_lde), _ints(zs_lde)
    pi_hash, betas, gammas, alphas = ([int(v) % P for v in a] for a in (pi_hash, betas, gammas, alphas))
    deltas = None if deltas is None else [int(v) % P for v in deltas]
    N = 1 << (shape.degree_bits + 3)
    assert len(cs) == shape.num_constants + NUM_ROUTED and len(wires) == NUM_WIRES and len(zs) == 20 + 2 * shape.num_lookup_polys
    assert all(len(col) == N for col in cs + wires + zs) and (deltas is None) == (shape.num_lookup_polys == 0)
    out = [[0] * N, [0] * N]
    for i in range(N):
        terms, z_h = vanishing_terms(shape, i, cs, wires, zs, pi_hash, betas, gammas, deltas)
        z_h_inv = pow(z_h, P - 2, P)
        for b in range(2):
            acc = 0
            for t in reversed(terms):                   # reduce_with_powers_multi (plonk_common.rs:97-114)
                acc = (acc * alphas[b] + t) % P
            out[b][i] = acc * z_h_inv % P
    return out
