"""An independent builder and model for circuits over the four extension-field arithmetic gates (no tests here).

Plain Python integers: F_p^2 = F_p[X]/(X^2 - 7) arithmetic, witness generators written from the reference's generator code
(gates/arithmetic_extension.rs:180-222, gates/multiplication_extension.rs:167-203, gates/reducing.rs:199-226,
gates/reducing_extension.rs:199-220), the gate list sorted as circuit_builder.rs:987 sorts it, the selector groups of
gates/selectors.rs:111-170 and copy-constraint classes from a union-find over the routed wires.  The product is imported only to fill
a CircuitDesc.
"""
import numpy as np

P = 2**64 - 2**32 + 1
W = 7                                   # Extendable<2>::W (field/src/goldilocks_extensions.rs:19)
UNUSED_SELECTOR = 2**32 - 1             # gates/selectors.rs:14
NUM_WIRES, NUM_ROUTED = 135, 80

# gl_circuit_desc gate codes (include/plonky2_mi355x.h)
NOOP, CONSTANT, PUBLIC_INPUT, ARITHMETIC = 0, 1, 2, 3
ARITHMETIC_EXT, MUL_EXT, REDUCING, REDUCING_EXT = 10, 11, 12, 13
# (degree, Debug id) per gate: the sort key of circuit_builder.rs:987
GATE_KEY = {
    NOOP: (0, "NoopGate"),
    CONSTANT: (1, "ConstantGate { num_consts: 2 }"),
    PUBLIC_INPUT: (1, "PublicInputGate"),
    REDUCING_EXT: (2, "ReducingExtensionGate { num_coeffs: 32 }"),
    REDUCING: (2, "ReducingGate { num_coeffs: 43 }"),
    ARITHMETIC_EXT: (3, "ArithmeticExtensionGate { num_ops: 10 }"),
    ARITHMETIC: (3, "ArithmeticGate { num_ops: 20 }"),
    MUL_EXT: (3, "MulExtensionGate { num_ops: 13 }"),
}
ARITH_EXT_OPS, MUL_EXT_OPS, REDUCING_COEFFS, REDUCING_EXT_COEFFS = 80 // 8, 80 // 6, min(80 - 6, (135 - 4) // 3), min((80 - 6) // 2, (135 - 4) // 4)
NUM_CONSTRAINTS = {ARITHMETIC_EXT: 2 * ARITH_EXT_OPS, MUL_EXT: 2 * MUL_EXT_OPS, REDUCING: 2 * REDUCING_COEFFS, REDUCING_EXT: 2 * REDUCING_EXT_COEFFS}
# DefaultGateSerializer position and the usize that follows it (util/serialization/gate_serialization.rs:90-106)
SERIAL_TAG = {ARITHMETIC_EXT: (1, ARITH_EXT_OPS), MUL_EXT: (8, MUL_EXT_OPS), REDUCING_EXT: (14, REDUCING_EXT_COEFFS), REDUCING: (15, REDUCING_COEFFS)}


# ------------------------------------------------------------------------------- F_p^2
def ext_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def ext_mul(x, y):
    return ((x[0] * y[0] + W * x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def ext_scale(x, s):
    return (x[0] * s % P, x[1] * s % P)


def ext_pow(x, k):
    r = (1, 0)
    while k:
        if k & 1:
            r = ext_mul(r, x)
        x, k = ext_mul(x, x), k >> 1
    return r


def horner(coeffs, x, start=(0, 0)):
    """start x^len + sum_i coeffs[i] x^(len - 1 - i): what a chain of reducing steps computes (util/reducing.rs)."""
    acc = start
    for c in coeffs:
        acc = ext_add(ext_mul(acc, x), c)
    return acc


# ------------------------------------------------------------------------------- wire layouts and generators
def reducing_acc_wire(gate, i):
    """first wire of accumulator i; the last accumulator is the output (reducing.rs:49-55, reducing_extension.rs:51-58)"""
    nc = REDUCING_COEFFS if gate == REDUCING else REDUCING_EXT_COEFFS
    start = 6 + nc * (1 if gate == REDUCING else 2)
    return 0 if i == nc - 1 else start + 2 * i


def reducing_coeff_wire(gate, i):
    return 6 + i if gate == REDUCING else 6 + 2 * i


class Circuit:
    """Rows of (gate, two constants, 135 wire values) and a union-find over routed wires (row, column)."""

    def __init__(self):
        self.rows, self.parent = [], {}

    def add_row(self, gate, consts=(0, 0)):
        self.rows.append([gate, list(consts), [0] * NUM_WIRES])
        return len(self.rows) - 1

    def put(self, row, col, ext):
        """an extension element on wires col, col + 1"""
        self.rows[row][2][col], self.rows[row][2][col + 1] = ext[0] % P, ext[1] % P

    def get(self, row, col):
        return (self.rows[row][2][col], self.rows[row][2][col + 1])

    def _find(self, x):
        while self.parent.setdefault(x, x) != x:
            self.parent[x] = self.parent[self.parent[x]]
            x = self.parent[x]
        return x

    def connect(self, a, b, width=1):
        """copy constraint between routed wires a = (row, col) and b, `width` adjacent wires"""
        for k in range(width):
            x, y = (a[0], a[1] + k), (b[0], b[1] + k)
            assert x[1] < NUM_ROUTED and y[1] < NUM_ROUTED
            assert self.rows[x[0]][2][x[1]] == self.rows[y[0]][2][y[1]], "copy constraint between unequal wires"
            self.parent[self._find(x)] = self._find(y)

    # -- one gate row each: the operands go in, the generator's outputs are written; returns the row
    def arithmetic_ext_row(self, c0, c1, ops):
        """ops: up to 10 of (m0, m1, addend); output = c0 m0 m1 + c1 addend (arithmetic_extension.rs:199-221)"""
        r = self.add_row(ARITHMETIC_EXT, (c0, c1))
        for i, (m0, m1, ad) in enumerate(ops):
            self.put(r, 8 * i, m0); self.put(r, 8 * i + 2, m1); self.put(r, 8 * i + 4, ad)
            self.put(r, 8 * i + 6, ext_add(ext_scale(ext_mul(m0, m1), c0), ext_scale(ad, c1)))
        return r

    def mul_ext_row(self, c0, ops):
        """ops: up to 13 of (m0, m1); output = c0 m0 m1 (multiplication_extension.rs:186-202)"""
        r = self.add_row(MUL_EXT, (c0, 0))
        for i, (m0, m1) in enumerate(ops):
            self.put(r, 6 * i, m0); self.put(r, 6 * i + 2, m1)
            self.put(r, 6 * i + 4, ext_scale(ext_mul(m0, m1), c0))
        return r

    def reducing_row(self, gate, alpha, old_acc, coeffs):
        """coeffs: exactly 43 base elements (REDUCING) or 32 extension elements (REDUCING_EXT), zero-padded by the caller as
        ReducingFactorTarget does; acc_i = acc_(i-1) alpha + coeff_i (reducing.rs:219-225)"""
        nc = REDUCING_COEFFS if gate == REDUCING else REDUCING_EXT_COEFFS
        assert len(coeffs) == nc
        r = self.add_row(gate)
        self.put(r, 2, alpha); self.put(r, 4, old_acc)
        acc = old_acc
        for i, c in enumerate(coeffs):
            if gate == REDUCING:
                self.rows[r][2][6 + i] = c % P
                c = (c, 0)
            else:
                self.put(r, 6 + 2 * i, c)
            acc = ext_add(ext_mul(acc, alpha), c)
            self.put(r, reducing_acc_wire(gate, i), acc)
        return r

    def arithmetic_row(self, c0, c1, ops):
        """the base ArithmeticGate: ops of (m0, m1, addend), output = c0 m0 m1 + c1 addend (arithmetic_base.rs)"""
        r = self.add_row(ARITHMETIC, (c0, c1))
        for i, (m0, m1, ad) in enumerate(ops):
            w = self.rows[r][2]
            w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3] = m0 % P, m1 % P, ad % P, (c0 * m0 * m1 + c1 * ad) % P
        return r

    # -- build(): public-input row tied to a ConstantGate zero, NoopGate padding, gate list, selectors, constants, classes
    def finish(self, min_degree_bits=3, hasher=0):
        from plonky2_demo_amd._lib import CircuitDesc
        const_row = self.add_row(CONSTANT, (0, 1))           # wires 0, 1 = the constants 0, 1
        self.rows[const_row][2][1] = 1
        pi_row = self.add_row(PUBLIC_INPUT)                  # zero public inputs: their hash is [0; 4]
        for k in range(4):
            self.connect((pi_row, k), (const_row, 0))
        lg = max(min_degree_bits, (len(self.rows) - 1).bit_length())
        n = 1 << lg
        while len(self.rows) < n:
            self.add_row(NOOP)
        gates = sorted({r[0] for r in self.rows}, key=lambda g: GATE_KEY[g])
        degree = [GATE_KEY[g][0] for g in gates]
        max_degree = 8 + 1
        if degree[-1] + len(gates) - 1 <= max_degree:
            groups = [(0, len(gates))]
        else:
            groups, start = [], 0
            while start < len(gates):
                size = 0
                while start + size < len(gates) and size + degree[start + size] < max_degree:
                    size += 1
                groups.append((start, start + size))
                start += size
        group_of = [next(k for k, (s, e) in enumerate(groups) if s <= i < e) for i in range(len(gates))]

        d = CircuitDesc()
        d.degree_bits, d.num_wires, d.num_routed_wires, d.num_challenges, d.quotient_degree_factor = lg, NUM_WIRES, NUM_ROUTED, 2, 8
        d.num_selectors, d.num_constants = len(groups), len(groups) + 2
        # standard_recursion_config (plonk/circuit_data.rs:72-90); ConstantArityBits(4, 5) (fri/reduction_strategies.rs:39-49)
        d.rate_bits, d.cap_height, d.proof_of_work_bits, d.num_query_rounds = 3, 4, 16, 28
        rounds, db = 0, lg
        while db > 5 and db + d.rate_bits - 4 >= d.cap_height:
            d.fri_arity_bits[rounds] = 4
            rounds, db = rounds + 1, db - 4
        d.num_fri_rounds, d.num_public_inputs, d.num_gates, d.hasher = rounds, 0, len(gates), hasher
        for i, g in enumerate(gates):
            d.gate_types[i], d.gate_selector_index[i] = g, group_of[i]
            d.gate_group_start[i], d.gate_group_end[i] = groups[group_of[i]]
        x = 1
        for j in range(NUM_ROUTED):                           # get_unique_coset_shifts: 7^j (field/src/cosets.rs:9-24)
            d.k_is[j], x = x, x * 7 % P

        constants = np.zeros((d.num_constants, n), dtype=np.uint64)
        for r, (g, consts, _) in enumerate(self.rows):
            i = gates.index(g)
            for s in range(len(groups)):
                constants[s, r] = i if group_of[i] == s else UNUSED_SELECTOR
            constants[len(groups), r], constants[len(groups) + 1, r] = consts[0] % P, consts[1] % P
        # class id of a wire = the position of its class's root; a wire in no copy constraint is its own root
        classes = (np.arange(NUM_ROUTED, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :])
        for (r, c) in list(self.parent):
            root = self._find((r, c))
            classes[c, r] = root[1] * n + root[0]
        self.desc, self.constants, self.classes, self.n = d, constants, classes, n
        return self

    def wires(self):
        out = np.zeros((NUM_WIRES, len(self.rows)), dtype=np.uint64)
        for r, (_, _, w) in enumerate(self.rows):
            out[:, r] = np.array(w, dtype=np.uint64)
        return out


# ------------------------------------------------------------------------------- the two families
EDGES = [0, 1, P - 1]


class _Rng:
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def base(self):
        return (int(self.rs.randint(0, 2**32)) * 2**32 + int(self.rs.randint(0, 2**32))) % P

    def ext(self):
        return (self.base() % P, self.base() % P)


def isolated(gates, seed, rows_per_gate=2, min_degree_bits=3):
    """rows_per_gate rows of every gate in `gates`, every operand independent (every wire class outside the public-input row a
    singleton), random from `seed` with 0, 1, p - 1 and (p - 1, p - 1) among the operands and constants.  -> Circuit (finished)"""
    rng, c = _Rng(seed), Circuit()
    special = [(0, 0), (1, 0), (P - 1, 0), (P - 1, P - 1), (0, 1), (0, P - 1)]

    def operand(k):
        return special[k % len(special)] if k < len(special) else rng.ext()

    for g in gates:
        for rep in range(rows_per_gate):
            consts = (EDGES[rep % 3], EDGES[(rep + 2) % 3]) if rep < rows_per_gate - 1 else (rng.base() % P, rng.base() % P)
            if g == ARITHMETIC_EXT:
                c.arithmetic_ext_row(consts[0], consts[1], [(operand(3 * i + rep), rng.ext(), operand(3 * i + 1 + rep)) for i in range(ARITH_EXT_OPS)])
            elif g == MUL_EXT:
                c.mul_ext_row(consts[1] if rep == 0 else consts[0], [(operand(2 * i + rep), operand(13 - i) if i % 2 else rng.ext()) for i in range(MUL_EXT_OPS)])
            elif g == REDUCING:
                coeffs = [EDGES[i % 3] if i < 6 else rng.base() % P for i in range(REDUCING_COEFFS)]
                c.reducing_row(g, rng.ext() if rep else (P - 1, P - 1), operand(rep + 2), coeffs)
            else:
                c.reducing_row(g, rng.ext() if rep else (P - 1, P - 1), operand(rep + 2), [operand(i) for i in range(REDUCING_EXT_COEFFS)])
    return c.finish(min_degree_bits=min_degree_bits)


def constraint_cell(gate, j):
    """a wire that constraint j of `gate` reads: the output / accumulator component it checks; for the ReducingGate's component 0 the
    base-field coefficient"""
    i, comp = divmod(j, 2)
    if gate == ARITHMETIC_EXT:
        return 8 * i + 6 + comp
    if gate == MUL_EXT:
        return 6 * i + 4 + comp
    if gate == REDUCING and comp == 0:
        return reducing_coeff_wire(gate, i)
    return reducing_acc_wire(gate, i) + comp


class Chained:
    """All four gates, outputs routed into later operands across rows and gate types, with ArithmeticGate, ConstantGate,
    PublicInputGate and NoopGate rows: eight gate types, two selector groups.  `results` holds (name, output wires' value, the
    model's direct value)."""

    def __init__(self, seed=1, min_degree_bits=4, hasher=0):
        rng, c = _Rng(seed), Circuit()
        self.results = []
        x = rng.ext()
        # x^k, k = 2 * 13 + 1: two MulExtensionGate rows, each op multiplies the previous output by x
        k, prev, prev_at, x_at = 1, x, None, None
        for _ in range(2):
            ops, acc = [], prev
            for i in range(MUL_EXT_OPS):
                ops.append((acc, x))
                acc = ext_mul(acc, x)
            r = c.mul_ext_row(1, ops)
            if x_at is None:
                x_at = (r, 2)                                      # x lives on the first m1; the first m0 is x too
                c.connect((r, 0), x_at, 2)
            else:
                c.connect((r, 0), prev_at, 2)                      # m0 = the previous row's last output
            for i in range(MUL_EXT_OPS):
                if (r, 6 * i + 2) != x_at:
                    c.connect((r, 6 * i + 2), x_at, 2)             # m1 = x everywhere
                if i:
                    c.connect((r, 6 * i), (r, 6 * (i - 1) + 4), 2)  # m0 = the previous output
            prev, prev_at, k = acc, (r, 6 * (MUL_EXT_OPS - 1) + 4), k + MUL_EXT_OPS
        self.results.append(("x^27 by MulExtensionGate", c.get(*prev_at), ext_pow(x, k)))
        mul_out = prev_at
        # a degree-10 polynomial at x by ArithmeticExtensionGate Horner steps: acc = 1 * acc * x + 1 * coeff; starts from x^27
        poly = [rng.ext() for _ in range(ARITH_EXT_OPS)]
        ops, acc = [], prev
        for co in poly:
            ops.append((acc, x, co))
            acc = ext_add(ext_mul(acc, x), co)
        r = c.arithmetic_ext_row(1, 1, ops)
        c.connect((r, 0), mul_out, 2)
        for i in range(ARITH_EXT_OPS):
            c.connect((r, 8 * i + 2), x_at, 2)
            if i:
                c.connect((r, 8 * i), (r, 8 * (i - 1) + 6), 2)
        horner_out = (r, 8 * (ARITH_EXT_OPS - 1) + 6)
        self.results.append(("Horner by ArithmeticExtensionGate", c.get(*horner_out), horner(poly, x, start=ext_pow(x, k))))
        # 60 base coefficients by two ReducingGate rows (43 + 17 zero-padded as ReducingFactorTarget::reduce_base pads), alpha = the Horner
        # output, the second row's old_acc = the first row's output
        alpha = c.get(*horner_out)
        base = [EDGES[i % 3] if i < 3 else rng.base() % P for i in range(60)]
        r1 = c.reducing_row(REDUCING, alpha, (0, 0), base[:43])
        rest = base[43:]
        r2 = c.reducing_row(REDUCING, alpha, c.get(r1, 0), rest + [0] * (43 - len(rest)))
        c.connect((r1, 2), horner_out, 2); c.connect((r2, 2), horner_out, 2); c.connect((r2, 4), (r1, 0), 2)
        want = ext_mul(horner([(b, 0) for b in base], alpha), ext_pow(alpha, 43 - len(rest)))      # the zero padding multiplies by alpha^26
        self.results.append(("60 base coefficients by ReducingGate", c.get(r2, 0), want))
        # 40 extension coefficients by two ReducingExtensionGate rows, alpha = x, old_acc of the first = the ReducingGate output
        coeffs = [rng.ext() for _ in range(40)]
        start = c.get(r2, 0)
        r3 = c.reducing_row(REDUCING_EXT, x, start, coeffs[:32])
        rest = coeffs[32:]
        r4 = c.reducing_row(REDUCING_EXT, x, c.get(r3, 0), rest + [(0, 0)] * (32 - len(rest)))
        c.connect((r3, 2), x_at, 2); c.connect((r4, 2), x_at, 2); c.connect((r3, 4), (r2, 0), 2); c.connect((r4, 4), (r3, 0), 2)
        want = ext_mul(horner(coeffs, x, start=start), ext_pow(x, 32 - len(rest)))
        self.results.append(("40 extension coefficients by ReducingExtensionGate", c.get(r4, 0), want))
        # ArithmeticGate: the two components of the last output multiplied and added, from copies of the output wires
        o = c.get(r4, 0)
        r5 = c.arithmetic_row(3, 5, [(o[0], o[1], o[0])])
        c.connect((r5, 0), (r4, 0)); c.connect((r5, 1), (r4, 1)); c.connect((r5, 2), (r4, 0))
        self.results.append(("ArithmeticGate", (c.rows[r5][2][3], 0), ((3 * o[0] * o[1] + 5 * o[0]) % P, 0)))
        self.circuit = c.finish(min_degree_bits=min_degree_bits, hasher=hasher)
