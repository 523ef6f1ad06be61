"""AIRs as expression DAGs, with generators of satisfying traces (no tests here).  Every AIR is written by a function of a builder, so
that it runs on stark_dag_model.Builder (the DAGs below) and on plonky2_demo_amd.StarkDagBuilder alike.

  CONVERTED    the twelve term-list AIRs of stark_airs.py, converted mechanically (dag_from_terms)
  sbox2        twelve state columns, two rounds per row of x -> M (x + c)^3 with a dense 12 x 12 M: degree 9, q = 8, rate_bits 3;
               first-row constraints against public inputs, a last-row constraint.  Its expansion passes GL_STARK_MAX_TERMS.
  at_cap       GL_STARK_DAG_MAX_LIVE distinct values live at once, then consumed in reverse order under distinct weights, so that two
               exchanged slots change the constraint; at_cap(129) is the sibling that is refused
  alias        chains in which the destination takes the slot of its dying a operand, of its dying b operand, and x * x with x dying
  operands     every op with every operand kind in each position; the non-canonical constants p, p + 1, 2^64 - 1; constraints that
               are a bare LOCAL, NEXT, PUBLIC, CONST operand; one node behind two constraints; a dead node; nodes defined out of
               constraint order
  BOUND        one AIR per filter whose constraint sits exactly on the degree bound, at q = 1, 3 and 8
"""
import numpy as np

import stark_airs
import stark_dag_model as dm
from stark_airs import ALL, FIRST_ROW, LAST_ROW, LOCAL, NEXT, P, TRANSITION

FILTER_CALL = {ALL: "constraint", TRANSITION: "constraint_transition", FIRST_ROW: "constraint_first_row", LAST_ROW: "constraint_last_row"}


def _draw(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def _rows_to_columns(rows):
    return np.array(rows, dtype=np.uint64).T.copy()


# ------------------------------------------------------------------------------- the term lists, converted
def write_terms(b, air):
    """sum coeff prod operand, literally: every term a chain of products from its coefficient, every constraint a chain of sums"""
    leaf = {LOCAL: b.local, NEXT: b.next, stark_airs.PUBLIC: b.public}
    for filt, terms in air.constraints:
        total = None
        for coeff, ops in terms:
            m = b.const(coeff)
            for kind, idx in ops:
                m = m * leaf[kind](idx)
            total = m if total is None else total + m
        getattr(b, FILTER_CALL[filt])(b.const(0) if total is None else total)


def dag_from_terms(air):
    b = dm.Builder(air.num_columns, air.num_public_inputs)
    write_terms(b, air)
    return dm.dag_air(air.name, air.num_columns, air.num_public_inputs, air.constraint_degree, air.rate_bits, b, air.pairs, air.trace)


CONVERTED = {name: dag_from_terms(air) for name, air in stark_airs.AIRS.items()}

# ------------------------------------------------------------------------------- sbox2
WIDTH = 12
SBOX_M = [[(7 * i * i + 3 * i * j + 5 * j * j + 11 * i + 13 * j + 1) % 251 + 1 for j in range(WIDTH)] for i in range(WIDTH)]      # dense: no zero entry
SBOX_C = [[(1 << 40) + 97 * r + 31 * j * j + j for j in range(WIDTH)] for r in range(2)]


def sbox_round(state, r):
    cubes = [pow((x + c) % P, 3, P) for x, c in zip(state, SBOX_C[r])]
    return [sum(m * s for m, s in zip(row, cubes)) % P for row in SBOX_M]


def write_sbox2(b):
    state = [b.local(j) for j in range(WIDTH)]
    for j in range(WIDTH):
        b.constraint_first_row(state[j] - b.public(j))
    for r in range(2):
        cubes = []
        for j in range(WIDTH):
            t = state[j] + SBOX_C[r][j]
            cubes.append(t * t * t)
        nxt = []
        for i in range(WIDTH):
            acc = cubes[0] * SBOX_M[i][0]
            for j in range(1, WIDTH):
                acc = acc + cubes[j] * SBOX_M[i][j]
            nxt.append(acc)
        state = nxt
    for i in range(WIDTH):
        b.constraint_transition(b.next(i) - state[i])
    b.constraint_last_row(b.local(0) - b.public(WIDTH))


def _sbox2_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(11000 + seed))
    state = [int(v) for v in _draw(rng, WIDTH)]
    rows = []
    for _ in range(n):
        rows.append(state)
        state = sbox_round(sbox_round(state, 0), 1)
    return _rows_to_columns(rows), rows[0] + [rows[n - 1][0]]


def _built(name, num_columns, num_public_inputs, constraint_degree, rate_bits, write, trace, pairs=()):
    b = dm.Builder(num_columns, num_public_inputs)
    write(b)
    return dm.dag_air(name, num_columns, num_public_inputs, constraint_degree, rate_bits, b, [list(p) for p in pairs], trace)


sbox2 = _built("sbox2", WIDTH, WIDTH + 1, 9, 3, write_sbox2, _sbox2_trace)


# ------------------------------------------------------------------------------- at_cap
def write_at_cap(live):
    def write(b):
        # `live` distinct values of degree 1, all live when the last is defined ...
        values = [b.local(0) * (j + 2) for j in range(live - 1)] + [b.local(1) * (live + 1)]
        # ... then consumed last to first, each under another power of 7: exchanging two slots changes the sum
        acc = values[-1]
        for v in reversed(values[:-1]):
            acc = acc * 7 + v
        b.constraint(b.local(2) - acc)
    return write


def _at_cap_trace(live):
    def trace(n, seed=0):
        rng = np.random.Generator(np.random.PCG64(12000 + seed))
        x, y = ([int(v) for v in _draw(rng, n)] for _ in range(2))
        z = []
        for i in range(n):
            values = [x[i] * (j + 2) % P for j in range(live - 1)] + [y[i] * (live + 1) % P]
            acc = values[-1]
            for v in reversed(values[:-1]):
                acc = (acc * 7 + v) % P
            z.append(acc)
        return np.array([x, y, z], dtype=np.uint64), []
    return trace


def at_cap(live=dm.MAX_LIVE):
    return _built("at_cap%d" % live, 3, 0, 2, 1, write_at_cap(live), _at_cap_trace(live))


# ------------------------------------------------------------------------------- alias
def write_alias(b):
    keep = b.local(1) - b.local(2)              # slot 0 for the whole program: the chains below run in the slots above it
    t = b.local(0) + b.local(1)                 # destination = the slot of the dying a operand, three times
    t = t * b.local(2)
    t = t + b.next(0)
    t = t - 9
    u = b.local(1) * b.local(2)                 # destination = the slot of the dying b operand, three times (t stays live beside it)
    u = b.local(0) - u
    u = 3 * u
    u = b.next(1) + u
    w = b.local(0) + b.local(2)                 # x * x with x dying: one slot given back once
    w = w * w
    b.constraint(b.local(3) - (((t + u) + w) + keep))


def _alias_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(13000 + seed))
    c = [[int(v) for v in _draw(rng, n)] for _ in range(3)]
    out = []
    for i in range(n):
        x0, x1, x2, n0, n1 = c[0][i], c[1][i], c[2][i], c[0][(i + 1) % n], c[1][(i + 1) % n]       # an ALL constraint reads row 0 after the last row
        t = ((x0 + x1) * x2 + n0 - 9) % P
        u = (n1 + 3 * (x0 - x1 * x2)) % P
        out.append((t + u + (x0 + x2) ** 2 + x1 - x2) % P)
    return np.array(c + [out], dtype=np.uint64), []


alias = _built("alias", 4, 0, 3, 1, write_alias, _alias_trace)

# ------------------------------------------------------------------------------- operands
NON_CANONICAL = [P, P + 1, 2**64 - 1]
OPERANDS_COLUMNS = 6          # 0, 1 free; 2 the sum's value; 3 zero; 4 = column 0 - column 1; 5 = column 0 column 1 + public 1


def _operand_leaves(b, node):
    """one operand of every kind; the CONST one is non-canonical"""
    return [b.local(0), b.next(1), b.public(1), node, b.const(NON_CANONICAL[2])]


def write_operands(b):
    dead = b.local(3) * b.local(3) * b.next(0)                              # two dead nodes, one behind the other
    assert dead is not None
    node = b.local(1) + b.next(0)                                          # the NODE operand, of degree 1
    late = b.local(0) * b.local(1) + b.public(1) - b.local(5)              # defined first, consumed last: the scheduler holds its constraint back
    total, weight = None, 1
    for op in ("add", "sub", "mul"):
        for a in _operand_leaves(b, node):
            for c in _operand_leaves(b, node):
                r = a + c if op == "add" else a - c if op == "sub" else a * c
                weight += 1
                total = r * weight if total is None else total + r * weight
    total = total + b.const(NON_CANONICAL[0]) + b.const(NON_CANONICAL[1])
    b.constraint(b.local(2) - total)
    b.constraint(b.local(3))                                               # bare operands
    b.constraint_transition(b.next(3))
    b.constraint_first_row(b.public(0))
    b.constraint_last_row(b.const(NON_CANONICAL[0]))
    shared = b.local(4) - (b.local(0) - b.local(1))                        # one node behind two constraints
    b.constraint(shared)
    b.constraint_transition(shared)
    b.constraint(late)


def _operands_trace(n, seed=0):
    rng = np.random.Generator(np.random.PCG64(14000 + seed))
    x, y = ([int(v) for v in _draw(rng, n)] for _ in range(2))
    pis = [P, int(_draw(rng, 1)[0])]                                       # public 0 is zero, written non-canonically
    cols = [x, y, [], [0] * n, [(a - c) % P for a, c in zip(x, y)], [(a * c + pis[1]) % P for a, c in zip(x, y)]]
    for i in range(n):
        node = (y[i] + x[(i + 1) % n]) % P
        leaves = [x[i], y[(i + 1) % n], pis[1], node, NON_CANONICAL[2] % P]
        total, weight = 0, 1
        for op in ("add", "sub", "mul"):
            for a in leaves:
                for c in leaves:
                    weight += 1
                    total += (a + c if op == "add" else a - c if op == "sub" else a * c) * weight
        cols[2].append((total + NON_CANONICAL[0] + NON_CANONICAL[1]) % P)
    return np.array(cols, dtype=np.uint64), pis


operands = _built("operands", OPERANDS_COLUMNS, 2, 3, 1, write_operands, _operands_trace)


# ------------------------------------------------------------------------------- on the degree bound
def _power(e, d):
    r = e
    for _ in range(d - 1):
        r = r * e
    return r


def bound_air(filt, q):
    """columns x, k; the one constraint has degree q + 1 under ALL / TRANSITION, q under FIRST_ROW / LAST_ROW"""
    d = q if filt in (FIRST_ROW, LAST_ROW) else q + 1
    order = d - 1                                                          # ALL: x^d = x, x zero or a root of unity of order d - 1 (1, 3, 8 divide 2^32 - 1 or are 2^k)
    roots = [0] + [pow(7, (P - 1) // order * i, P) for i in range(order)] if filt == ALL else []
    assert all(pow(r, d, P) == r for r in roots)

    def write(b):
        x = b.local(0)
        if filt == ALL:
            b.constraint(_power(x, d) - x)
        elif filt == TRANSITION:
            b.constraint_transition(b.next(0) - _power(x, d) - b.local(1))
        elif filt == FIRST_ROW:
            b.constraint_first_row(_power(x, d) - b.public(0))
        else:
            b.constraint_last_row(_power(x, d) - b.public(0))

    def trace(n, seed=0):
        rng = np.random.Generator(np.random.PCG64(15000 + 16 * q + filt + 64 * seed))
        k = [int(v) for v in _draw(rng, n)]
        if filt == ALL:
            xs = [roots[int(v)] for v in rng.integers(0, len(roots), size=n)]
        elif filt == TRANSITION:
            xs = [int(_draw(rng, 1)[0])]
            for i in range(n - 1):
                xs.append((pow(xs[-1], d, P) + k[i]) % P)
        else:
            xs = [int(v) for v in _draw(rng, n)]
        return np.array([xs, k], dtype=np.uint64), [pow(xs[0 if filt == FIRST_ROW else n - 1], d, P)]
    return _built("bound-%s-q%d" % (FILTER_CALL[filt], q), 2, 1, q + 1 if q > 1 else 2, (q - 1).bit_length() or 1, write, trace)


BOUND = {a.name: a for a in (bound_air(f, q) for q in (1, 3, 8) for f in (ALL, TRANSITION, FIRST_ROW, LAST_ROW))}
OWN = {a.name: a for a in [sbox2, at_cap(), alias, operands] + list(BOUND.values())}
EVERY = dict(list(CONVERTED.items()) + list(OWN.items()))


# ------------------------------------------------------------------------------- the table set of stark_ctl_airs.py, some tables as DAGs
def api_set(p, lgs, config, dag_tables=None, tables=None, hasher="poseidon"):
    """stark_ctl_airs.api_set with the tables named in dag_tables (default: `mul`) converted to DAGs, the others left as term lists"""
    import stark_ctl_airs as ca
    tables = ca.TABLES if tables is None else tables
    desc = ca.api_set(p, tables, ca.LOOKUPS, lgs, config, hasher=hasher)
    for t in ((ca.MUL,) if dag_tables is None else dag_tables):
        desc.tables[t] = (dm.desc_of(p, dag_from_terms(tables[t])), desc.tables[t][1])
    return desc
