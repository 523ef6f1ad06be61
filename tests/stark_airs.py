"""Four AIRs as term lists, with generators of satisfying traces (no tests here).

An AIR is plain data in the shape plonky2_demo_amd.StarkDesc takes: constraints = [(filter, [(coeff, [(kind, index), ...]), ...]), ...],
pairs = [[(lhs, rhs), ...], ...].  trace(n, seed) -> (columns [num_columns][n] as uint64, public inputs).

  fibonacci  the reference's FibonacciStark (starky/src/fibonacci_stark.rs): q = 1, all three row filters, two Z polynomials
  cubic      x' = x^3 + k with a constants column, ONE pair of TWO column pairs: q = 2, one Z of two instances, beta powers
  quartic    degree 4, three pairs, an unfiltered boolean constraint, a PUBLIC factor and a constant term: q = 3 (no power of two)
  wide       130 columns, degree 2, no pairs: the two-oracle instance, more columns than a wave has lanes
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


def _air(name, num_columns, num_public_inputs, constraint_degree, rate_bits, constraints, pairs, trace):
    q = max(1, constraint_degree - 1)
    return SimpleNamespace(name=name, num_columns=num_columns, num_public_inputs=num_public_inputs, constraint_degree=constraint_degree,
                           rate_bits=rate_bits, constraints=constraints, pairs=pairs, trace=trace, q=q, qdb=(q - 1).bit_length())


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
], [[(2, 3)]], _fibonacci_trace)


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

AIRS = {a.name: a for a in (fibonacci, cubic, quartic, wide)}
