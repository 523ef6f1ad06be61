"""A system of three tables tied by two cross-table lookups, as data, with a generator of consistent traces (no tests here).

  ops    (table 0)  columns a b c s0 s1 u w: (s0 + s1)(a b - c) = 0, s0 and s1 boolean and never both.  Degree 3, q = 2.
  ops2   (table 1)  the same constraints on a b c s0 s1 and ONE permutation pair (p0, p1): its CTL Z comes after a permutation Z.  Another
                    degree_bits than ops.
  mul    (table 2)  columns a b c used b0 b1 b2 b3 t: used (a b - c) = 0, used boolean.  Degree 3.
  lookup 0   ops and ops2 look [a, b, c] up in mul; the looking filter is the LINEAR COMBINATION s0 + s1, the looked filter is `used`
  lookup 1   no filter on either side; mul is the LOOKING table -- so it is both looking and looked -- with the columns
             [le_bits(b0..b3), 3 t + 7] (a Column with a constant), looked up in ops' [u, w]
TABLES5 is the same system with a mul table of degree 5 (used^5 = used besides) under rate_bits 2: tables of q = 2 and of q = 4 in one
set, the first on every second point of the LDE.
An AIR has stark_airs' shape; a Column is (terms, constant), a TableWithColumns a namespace (table, columns, filter), a lookup a pair
(looking list, looked): what stark_ctl_model takes.
"""
from types import SimpleNamespace

import numpy as np

from stark_airs import ALL, L, M1, P, _air

OPS, OPS2, MUL = range(3)


def single(c):
    return ([(c, 1)], 0)


def le_bits(cs):
    return ([(c, 1 << k) for k, c in enumerate(cs)], 0)


def twc(table, columns, filter_column=None):
    return SimpleNamespace(table=table, columns=list(columns), filter=filter_column)


_OPS_CONSTRAINTS = [
    (ALL, [(1, [L(3), L(0), L(1)]), (1, [L(4), L(0), L(1)]), (M1, [L(3), L(2)]), (M1, [L(4), L(2)])]),     # (s0 + s1)(a b - c)
    (ALL, [(1, [L(3), L(3)]), (M1, [L(3)])]),
    (ALL, [(1, [L(4), L(4)]), (M1, [L(4)])]),
    (ALL, [(1, [L(3), L(4)])]),
]
_MUL_CONSTRAINTS = [
    (ALL, [(1, [L(3), L(0), L(1)]), (M1, [L(3), L(2)])]),                                                  # used (a b - c)
    (ALL, [(1, [L(3), L(3)]), (M1, [L(3)])]),
]
RATE_BITS = 1

ops = _air("ops", 7, 0, 3, RATE_BITS, _OPS_CONSTRAINTS, [], None)
ops2 = _air("ops2", 7, 0, 3, RATE_BITS, _OPS_CONSTRAINTS, [[(5, 6)]], None)
mul = _air("mul", 9, 0, 3, RATE_BITS, _MUL_CONSTRAINTS, [], None)
TABLES = [ops, ops2, mul]

# the variant: one more constraint on mul, five trace factors on every row (q + 1 at q = 4); every table at the set's rate_bits 2
RATE_BITS5 = 2
mul5 = _air("mul5", 9, 0, 5, RATE_BITS5, _MUL_CONSTRAINTS + [(ALL, [(1, [L(3)] * 5), (M1, [L(3)])])], [], None)
TABLES5 = [_air("ops", 7, 0, 3, RATE_BITS5, _OPS_CONSTRAINTS, [], None), _air("ops2", 7, 0, 3, RATE_BITS5, _OPS_CONSTRAINTS, [[(5, 6)]], None), mul5]

FILTER_OPS = ([(3, 1), (4, 1)], 0)                  # s0 + s1
LOOKUPS = [
    ([twc(OPS, [single(0), single(1), single(2)], FILTER_OPS), twc(OPS2, [single(0), single(1), single(2)], FILTER_OPS)],
     twc(MUL, [single(0), single(1), single(2)], single(3))),
    ([twc(MUL, [le_bits([4, 5, 6, 7]), ([(8, 3)], 7)])],
     twc(OPS, [single(5), single(6)])),
]


def traces(lgs, seed=0):
    """consistent traces [ops, ops2, mul] of 2^lgs[t] rows each: every table satisfies its AIR and check_ctls accepts; ops and mul have
    the same number of rows (lookup 1 has no filter)"""
    assert lgs[OPS] == lgs[MUL]
    rng = np.random.Generator(np.random.PCG64(4000 + seed))
    n = [1 << lg for lg in lgs]
    active = [n[OPS] // 3, n[OPS2] // 4]
    assert sum(active) <= n[MUL]

    def rand(k):
        return [int(v) for v in rng.integers(0, P, size=k, dtype=np.uint64)]
    out, looked_rows = [], []
    for t, width in ((OPS, 7), (OPS2, 7)):
        cols = [rand(n[t]) for _ in range(width)]
        on = set(int(i) for i in rng.choice(n[t], size=active[t], replace=False))
        for i in range(n[t]):
            cols[3][i] = cols[4][i] = 0
            if i in on:
                cols[2][i] = cols[0][i] * cols[1][i] % P
                cols[3 + i % 2][i] = 1
                looked_rows.append((cols[0][i], cols[1][i], cols[2][i]))
        if t == OPS2:
            perm = rng.permutation(n[t])
            cols[6] = [cols[5][int(j)] for j in perm]
        out.append(cols)
    cols = [rand(n[MUL]) for _ in range(9)]
    used = [int(i) for i in rng.choice(n[MUL], size=len(looked_rows), replace=False)]
    cols[3] = [0] * n[MUL]
    for i, row in zip(used, looked_rows):
        cols[0][i], cols[1][i], cols[2][i], cols[3][i] = row + (1,)
    for k in range(4):
        cols[4 + k] = [int(v) for v in rng.integers(0, 2, size=n[MUL])]
    perm = rng.permutation(n[MUL])
    for j in range(n[OPS]):                          # ops' (u, w) are mul's (bits, 3 t + 7), row for row under a permutation
        i = int(perm[j])
        out[OPS][5][j] = sum(cols[4 + k][i] << k for k in range(4))
        out[OPS][6][j] = (3 * cols[8][i] + 7) % P
    out.append(cols)
    return [np.array(c, dtype=np.uint64) for c in out]


def remove_one_looked_row(trs):
    """the same traces with one used row of mul switched off: every table still satisfies its own AIR, lookup 0 no longer holds"""
    trs = [t.copy() for t in trs]
    i = int(np.flatnonzero(trs[MUL][3])[0])
    trs[MUL][3][i] = 0
    return trs


def api_set(p, tables, lookups, lgs, config, hasher="poseidon"):
    """the system as plonky2_demo_amd.StarkSetDesc takes it"""
    def col(c):
        return p.CtlColumn(c[0], c[1])

    def tw(t):
        return p.TableWithColumns(t.table, [col(c) for c in t.columns], None if t.filter is None else col(t.filter))
    descs = [(p.StarkDesc(a.num_columns, a.num_public_inputs, a.constraint_degree, a.constraints, a.pairs), lg) for a, lg in zip(tables, lgs)]
    return p.StarkSetDesc(descs, [p.CrossTableLookup([tw(t) for t in looking], tw(looked)) for looking, looked in lookups], config, hasher=hasher)


def config(p, nc, rate_bits=RATE_BITS):
    c = p.StarkConfig.standard_fast_config()
    c.num_challenges, c.rate_bits = nc, rate_bits
    return c
