"""AIRs as term lists, with generators of satisfying traces (no tests here).

An AIR is plain data in the shape plonky2_demo_amd.StarkDesc takes: constraints = [(filter, [(coeff, [(kind, index), ...]), ...]), ...],
pairs = [[(lhs, rhs), ...], ...].  trace(n, seed) -> (columns [num_columns][n] as uint64, public inputs).

  fibonacci  the reference's FibonacciStark (starky/src/fibonacci_stark.rs): q = 1, all three row filters, two Z polynomials
  cubic      x' = x^3 + k with a constants column, ONE pair of TWO column pairs: q = 2, one Z of two instances, beta powers
  quartic    degree 4, three pairs, an unfiltered boolean constraint, a PUBLIC factor and a constant term: q = 3 (no power of two)
  wide       130 columns, degree 2, no pairs: the two-oracle instance, more columns than a wave has lanes
and, from one generator (x' = x^d + k, a column b with b^d = b on every row, permuted columns), the shapes the four leave out:
  quintic    degree 5 at rate_bits 3: q = 4, qdb = 2, every second LDE point; three pairs, an ALL constraint of q + 1 trace factors
  sextic     degree 6: q = 5 under qdb = 3, a trim tail of 3 n; two pairs, a PUBLIC factor
  nonic      degree 9: q = 8, qdb = 3; three pairs, one of three column pairs; all four filters
  linear     constraint_degree 1 (q = 1): x' = 3 x + k, one pair
  pairs33    degree 2, 33 single-column pairs: 33 x num_challenges Z polynomials, more than a wave has lanes from num_challenges 2 on
  longpair   degree 3, ONE pair of 64 column pairs: beta^63; at num_challenges 3 three instances in two Zs, the last batch partial
  manyfactors  a term of 64 factors (62 PUBLIC, two trace) beside a term without factors, no pairs
  nopublic   the same recurrence without public inputs
`longest` is the largest number of trace factors in a term (q + 1 unless stated).
"""
from types import SimpleNamespace

import numpy as np

P = 0xFFFFFFFF00000001
ALL, TRANSITION, FIRST_ROW, LAST_ROW = range(4)
LOCAL, NEXT, PUBLIC = range(3)
L = lambda c: (LOCAL, c)          # noqa: E731
N = lambda c: (NEXT, c)           # noqa: E731
PUB = lambda i: (PUBLIC, i)       # noqa: E731
M1 = P - 1


def _air(name, num_columns, num_public_inputs, constraint_degree, rate_bits, constraints, pairs, trace, longest=None):
    q = max(1, constraint_degree - 1)
    return SimpleNamespace(name=name, num_columns=num_columns, num_public_inputs=num_public_inputs, constraint_degree=constraint_degree,
                           rate_bits=rate_bits, constraints=constraints, pairs=pairs, trace=trace, q=q, qdb=(q - 1).bit_length(),
                           longest=q + 1 if longest is None else longest)


def _columns(rows):
    return np.array(rows, dtype=np.uint64).T.copy()


def _fibonacci_trace(n, seed=0, x0=0, x1=1):
    rows, acc = [], [x0 % P, x1 % P, 0, 1]
    for _ in range(n):
        rows.append(list(acc))
        acc = [acc[1], (acc[0] + acc[1]) % P, (acc[2] + 1) % P, (acc[3] + 1) % P]
    rows[n - 1][3] = 0
    return _columns(rows), [x0 % P, x1 % P, rows[n - 1][1]]


fibonacci = _air("fibonacci", 4, 3, 2, 1, [
    (FIRST_ROW, [(1, [L(0)]), (M1, [PUB(0)])]),
    (FIRST_ROW, [(1, [L(1)]), (M1, [PUB(1)])]),
    (LAST_ROW, [(1, [L(1)]), (M1, [PUB(2)])]),
    (TRANSITION, [(1, [N(0)]), (M1, [L(1)])]),
    (TRANSITION, [(1, [N(1)]), (M1, [L(0)]), (M1, [L(1)])]),
], [[(2, 3)]], _fibonacci_trace, longest=1)


def _cubic_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    k = [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]
    a = [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]
    b = [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]
    perm = rng.permutation(n)
    x, rows = int(rng.integers(0, P, dtype=np.uint64)), []
    x0 = x
    for i in range(n):
        rows.append([x, k[i], a[i], b[i], a[perm[i]], b[perm[i]]])       # the ROWS (a, b) are permuted together
        x = (pow(x, 3, P) + k[i]) % P
    return _columns(rows), [x0]


cubic = _air("cubic", 6, 1, 3, 1, [
    (FIRST_ROW, [(1, [L(0)]), (M1, [PUB(0)])]),
    (TRANSITION, [(1, [N(0)]), (M1, [L(0), L(0), L(0)]), (M1, [L(1)])]),
], [[(2, 4), (3, 5)]], _cubic_trace)


def _quartic_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    bits = [int(v) for v in rng.integers(0, 2, size=n)]
    cols = [[int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)] for _ in range(3)]      # columns 2, 4, 5
    perms = [rng.permutation(n) for _ in range(3)]
    scale = int(rng.integers(0, P, dtype=np.uint64))
    x = int(rng.integers(0, P, dtype=np.uint64))
    xs = []
    for i in range(n):
        xs.append(x)
        x = (pow(x, 4, P) + scale * bits[i] + 5) % P
    rows = [[xs[i], bits[i], cols[0][i], cols[0][perms[0][i]], cols[1][i], cols[2][i], cols[1][perms[1][i]], cols[2][perms[1][i]], xs[perms[2][i]]]
            for i in range(n)]
    return _columns(rows), [scale, xs[0], xs[n - 1]]


quartic = _air("quartic", 9, 3, 4, 2, [
    (FIRST_ROW, [(1, [L(0)]), (M1, [PUB(1)])]),
    (ALL, [(1, [L(1), L(1)]), (M1, [L(1)])]),                                                     # b b - b on every row
    (TRANSITION, [(1, [N(0)]), (M1, [L(0), L(0), L(0), L(0)]), (M1, [PUB(0), L(1)]), (P - 5, [])]),
    (LAST_ROW, [(1, [L(0)]), (M1, [PUB(2)])]),
], [[(2, 3)], [(4, 6), (5, 7)], [(0, 8)]], _quartic_trace)

WIDE = 130


def _wide_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(3000 + seed))
    row = [int(v) for v in rng.integers(0, P, size=WIDE, dtype=np.uint64)]
    rows = []
    for _ in range(n):
        rows.append(row)
        row = [(row[c] * row[(c + 1) % WIDE] + c) % P for c in range(WIDE)]
    return _columns(rows), [rows[0][0]]


wide = _air("wide", WIDE, 1, 2, 1,
            [(FIRST_ROW, [(1, [L(0)]), (M1, [PUB(0)])])] +
            [(TRANSITION, [(1, [N(c)]), (M1, [L(c), L((c + 1) % WIDE)]), ((P - c) % P, [])]) for c in range(WIDE)],
            [], _wide_trace)



# ------------------------------------------------------------------------------- the power family
def _power_air(name, degree, rate_bits, pair_lens, seed0, scaled=False, boolean=False, last_row=False, x_pair=True, step=None):
    """Columns: 0 x, 1 k, (2 b), then per pair its lhs columns and its rhs columns (the same rows, permuted together); with x_pair the
    last pair is (x, x permuted) and pair_lens lists the others.  Constraints: x = PUB on the first row; (b^degree = b on every row);
    x' = x^degree + k on transitions (x' = 3 x + k for degree 1; k scaled by PUB(0) with `scaled`); k = 0 (and x = PUB) on the last row."""
    base = 3 if boolean else 2
    pairs, at = [], base
    for ln in pair_lens:
        pairs.append([(at + i, at + ln + i) for i in range(ln)])
        at += 2 * ln
    if x_pair:
        pairs.append([(0, at)])
        at += 1
    num_columns = at
    x0_pub = 1 if scaled else 0
    num_pis = 1 + x0_pub + (1 if last_row else 0)
    grow = (P - 3, [L(0)]) if degree == 1 else (M1, [L(0)] * degree)
    constraints = [(FIRST_ROW, [(1, [L(0)]), (M1, [PUB(x0_pub)])])]
    if boolean:
        constraints.append((ALL, [(1, [L(2)] * degree), (M1, [L(2)])]))
    constraints.append((TRANSITION, [(1, [N(0)]), grow, (M1, [PUB(0), L(1)] if scaled else [L(1)])]))
    constraints.append((LAST_ROW, [(1, [L(1)])]))          # no transition reads k on the last row: it is zero, so that every cell is bound
    if last_row:
        constraints.append((LAST_ROW, [(1, [L(0)]), (M1, [PUB(x0_pub + 1)])]))
    order = degree - 1                                   # b^degree = b: zero or a root of unity of order degree - 1 (4: 2^48, 8: 2^24)
    roots = [0] + [pow(2, (192 // order) * i, P) for i in range(order)] if boolean else []

    def trace(n, seed=0):
        rng = np.random.Generator(np.random.PCG64(seed0 + seed))
        draw = lambda: [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]      # noqa: E731
        k, scale, x = draw()[:-1] + [0], int(rng.integers(0, P, dtype=np.uint64)) if scaled else 1, int(rng.integers(0, P, dtype=np.uint64))
        xs = []
        for i in range(n):
            xs.append(x)
            x = ((3 * x if degree == 1 else pow(x, degree, P)) + scale * k[i]) % P
        cols = [xs, k] + ([[roots[int(v)] for v in rng.integers(0, len(roots), size=n)]] if boolean else [])
        for ln in pair_lens:
            lhs, perm = [draw() for _ in range(ln)], rng.permutation(n)
            cols += lhs + [[c[perm[i]] for i in range(n)] for c in lhs]
        if x_pair:
            perm = rng.permutation(n)
            cols.append([xs[perm[i]] for i in range(n)])
        return np.array(cols, dtype=np.uint64), ([scale] if scaled else []) + [xs[0]] + ([xs[n - 1]] if last_row else [])
    assert all(pow(r, degree, P) == r for r in roots)
    return _air(name, num_columns, num_pis, degree, rate_bits, constraints, pairs, trace, longest=max(degree, 1))


quintic = _power_air("quintic", 5, 3, [1, 1], 4000, boolean=True)
sextic = _power_air("sextic", 6, 3, [1], 5000, scaled=True)
nonic = _power_air("nonic", 9, 3, [1, 3], 6000, boolean=True, last_row=True)
linear = _power_air("linear", 1, 1, [1], 7000, x_pair=False)
pairs33 = _power_air("pairs33", 2, 1, [1] * 32, 8000)
longpair = _power_air("longpair", 3, 1, [64], 9000, x_pair=False)

NUM_MANY_PUBLIC = 5
MANY_PUBLIC = [PUB((7 * i) % NUM_MANY_PUBLIC if i % 3 else 0) for i in range(62)]      # every index, index 0 over and over


def _product_trace(num_public):
    def trace(n, seed=0):
        rng = np.random.Generator(np.random.PCG64(10000 + seed))
        k = [int(v) for v in rng.integers(0, P, size=n - 1, dtype=np.uint64)] + [0]
        pis = [int(v) for v in rng.integers(1, P, size=num_public, dtype=np.uint64)]
        scale = 1
        for _, i in (MANY_PUBLIC if num_public else []):
            scale = scale * pis[i] % P
        x, xs = int(rng.integers(0, P, dtype=np.uint64)), []
        for i in range(n):
            xs.append(x)
            x = (scale * x % P * k[i] + 5) % P
        return np.array([xs, k], dtype=np.uint64), pis
    return trace


# x' = (prod of 62 public inputs) x k + 5: the trace factors sit inside and at the end of the 64; k = 0 on the last row
manyfactors = _air("manyfactors", 2, NUM_MANY_PUBLIC, 2, 1,
                   [(TRANSITION, [(1, [N(0)]), (M1, MANY_PUBLIC[:31] + [L(0)] + MANY_PUBLIC[31:] + [L(1)]), (P - 5, [])]), (LAST_ROW, [(1, [L(1)])])],
                   [], _product_trace(NUM_MANY_PUBLIC))
nopublic = _air("nopublic", 2, 0, 2, 1, [(TRANSITION, [(1, [N(0)]), (M1, [L(0), L(1)]), (P - 5, [])]), (LAST_ROW, [(1, [L(1)])])], [], _product_trace(0))

AIRS = {a.name: a for a in (fibonacci, cubic, quartic, wide, quintic, sextic, nonic, linear, pairs33, longpair, manyfactors, nopublic)}
