"""A plain Python-integer model of STARK constraints as an expression DAG (gl_stark_dag, include/plonky2_mi355x.h; no tests here):
  check              the DAG's own rules and the degree rule, counted formally
  schedule           the scheduling and liveness definition: which nodes run, where each constraint is consumed, max live
  constraint_values  the constraints over stark_model.Base / Ext, evaluated ALONG the schedule with every value deleted after its last
                     use: a schedule that consumed a constraint late, or a liveness count that let a value go early, fails here
  eval_vanishing / quotient_values / verify   stark_model's own consumer, permutation checks and verifier around them
  expand             a DAG multiplied out to the term list of stark_airs.py
  Builder            writes a DAG as plonky2_demo_amd.StarkDagBuilder does (the same calls: an AIR written against one runs on the other)
A DAG AIR is a SimpleNamespace like those of stark_airs.py with nodes = [(op, a, b), ...], constants = [...], dag_constraints =
[(filter, operand), ...] in place of `constraints`; an operand is (kind, index).
"""
from types import SimpleNamespace

import numpy as np

import fri_openings_model as fom
import stark_model as sm
from stark_airs import ALL, FIRST_ROW, LAST_ROW, LOCAL, NEXT, PUBLIC, TRANSITION
from stark_model import Base, P
from vanishing_model import primitive_root

NODE, CONST = 3, 4
ADD, SUB, MUL = range(3)
MAX_NODES, MAX_CONSTANTS, MAX_LIVE, MAX_CONSTRAINTS, MAX_TERMS = 65536, 65536, 128, 4096, 65536
U64 = np.uint64


class Refused(Exception):
    pass


def dag_air(name, num_columns, num_public_inputs, constraint_degree, rate_bits, builder, pairs, trace):
    q = max(1, constraint_degree - 1)
    return SimpleNamespace(name=name, num_columns=num_columns, num_public_inputs=num_public_inputs, constraint_degree=constraint_degree, rate_bits=rate_bits,
                           nodes=list(builder.nodes), constants=list(builder.constants), dag_constraints=list(builder.constraints), pairs=pairs, trace=trace,
                           q=q, qdb=(q - 1).bit_length())


# ------------------------------------------------------------------------------- the builder
class Expr:
    __slots__ = ("b", "operand")

    def __init__(self, b, operand):
        self.b, self.operand = b, operand

    def __add__(self, o):
        return self.b.node(ADD, self, o)

    def __radd__(self, o):
        return self.b.node(ADD, o, self)

    def __sub__(self, o):
        return self.b.node(SUB, self, o)

    def __rsub__(self, o):
        return self.b.node(SUB, o, self)

    def __mul__(self, o):
        return self.b.node(MUL, self, o)

    def __rmul__(self, o):
        return self.b.node(MUL, o, self)


class Builder:
    def __init__(self, num_columns, num_public_inputs):
        self.num_columns, self.num_public_inputs = num_columns, num_public_inputs
        self.nodes, self.constants, self.constraints, self.node_of, self.const_of = [], [], [], {}, {}

    def local(self, c):
        return Expr(self, (LOCAL, c))

    def next(self, c):
        return Expr(self, (NEXT, c))

    def public(self, i):
        return Expr(self, (PUBLIC, i))

    def const(self, v):
        v = int(v) if 0 <= int(v) < 1 << 64 else int(v) % P
        if v not in self.const_of:
            self.const_of[v] = len(self.constants)
            self.constants.append(v)
        return Expr(self, (CONST, self.const_of[v]))

    def node(self, op, a, b):
        key = (op, (a if isinstance(a, Expr) else self.const(a)).operand, (b if isinstance(b, Expr) else self.const(b)).operand)
        if key not in self.node_of:
            self.node_of[key] = len(self.nodes)
            self.nodes.append(key)
        return Expr(self, (NODE, self.node_of[key]))

    def _constraint(self, filt, e):
        self.constraints.append((filt, (e if isinstance(e, Expr) else self.const(e)).operand))

    def constraint(self, e):
        self._constraint(ALL, e)

    def constraint_transition(self, e):
        self._constraint(TRANSITION, e)

    def constraint_first_row(self, e):
        self._constraint(FIRST_ROW, e)

    def constraint_last_row(self, e):
        self._constraint(LAST_ROW, e)


# ------------------------------------------------------------------------------- the rules
def degrees(dag):
    """the degree rule: LOCAL / NEXT 1, PUBLIC / CONST 0, ADD / SUB the maximum, MUL the sum -> (per node, per constraint)"""
    node = []

    def of(operand):
        kind, idx = operand
        return 1 if kind in (LOCAL, NEXT) else node[idx] if kind == NODE else 0
    for op, a, b in dag.nodes:
        node.append(of(a) + of(b) if op == MUL else max(of(a), of(b)))
    return node, [of(operand) for _, operand in dag.dag_constraints]


def check(dag):
    """the DAG's own rules (gl_stark_dag_check's, params aside): raises Refused naming the rule"""
    def operand(o, defined):
        kind, idx = o
        if kind not in (LOCAL, NEXT, PUBLIC, NODE, CONST):
            raise Refused("operand kind")
        limit = {LOCAL: dag.num_columns, NEXT: dag.num_columns, PUBLIC: dag.num_public_inputs, CONST: len(dag.constants), NODE: len(dag.nodes)}[kind]
        if not 0 <= idx < limit:
            raise Refused("index out of range")
        if kind == NODE and idx >= defined:
            raise Refused("no earlier node")
    if len(dag.nodes) > MAX_NODES or len(dag.constants) > MAX_CONSTANTS or not 1 <= len(dag.dag_constraints) <= MAX_CONSTRAINTS:
        raise Refused("count")
    for k, (op, a, b) in enumerate(dag.nodes):
        if op not in (ADD, SUB, MUL):
            raise Refused("op")
        operand(a, k)
        operand(b, k)
    for filt, o in dag.dag_constraints:
        if filt not in (ALL, TRANSITION, FIRST_ROW, LAST_ROW):
            raise Refused("filter")
        operand(o, len(dag.nodes))
    for (filt, _), d in zip(dag.dag_constraints, degrees(dag)[1]):
        if d > (dag.q if filt in (FIRST_ROW, LAST_ROW) else dag.q + 1):
            raise Refused("degree")
    if schedule(dag)[1] > MAX_LIVE:
        raise Refused("live")


def schedule(dag):
    """-> (program, max live): program = [("op", node) | ("emit", constraint), ...].  Nodes run in the given order, one no constraint
    reaches is dropped; constraint c is consumed at the first position -- before node 0, or right after a node -- at which its value
    exists and constraint c - 1 has been consumed.  live(k) = the values defined at or before node k whose last use is after node k."""
    nodes, cons = dag.nodes, dag.dag_constraints
    used = [False] * len(nodes)
    for _, (kind, idx) in cons:
        if kind == NODE:
            used[idx] = True
    for k in range(len(nodes) - 1, -1, -1):
        if used[k]:
            for kind, idx in nodes[k][1:]:
                if kind == NODE:
                    used[idx] = True
    program, c = [], 0

    def flush(defined):
        nonlocal c
        while c < len(cons) and (cons[c][1][0] != NODE or cons[c][1][1] < defined):
            program.append(("emit", c))
            c += 1
    flush(0)
    for k in range(len(nodes)):
        if used[k]:
            program.append(("op", k))
        flush(k + 1)
    assert c == len(cons)
    # last use of every node, as a position in the program
    last = {}
    for at, (what, i) in enumerate(program):
        for kind, idx in (nodes[i][1:] if what == "op" else [cons[i][1]]):
            if kind == NODE:
                last[idx] = at
    dying = {}
    for end in last.values():
        dying[end] = dying.get(end, 0) + 1
    live = max_live = 0
    for at, (what, _) in enumerate(program):
        live -= dying.get(at, 0)                     # a value whose last use is here is not used AFTER here: it does not count
        if what == "op":
            live += 1                                # the node itself: it is used (or it was dropped), so its last use is later
            max_live = max(max_live, live)
    return program, max_live


def num_instructions(dag):
    return len(schedule(dag)[0])


def constraint_values(F, dag, local, nxt, pub):
    """the constraints, unfiltered, in the order they are consumed (= the order given), evaluated along the schedule: a value is deleted
    after its last use, and never more than max live are held"""
    program, max_live = schedule(dag)
    last = {}
    for at, (what, i) in enumerate(program):
        for kind, idx in (dag.nodes[i][1:] if what == "op" else [dag.dag_constraints[i][1]]):
            if kind == NODE:
                last[idx] = at
    held, out = {}, []

    def value(o):
        kind, idx = o
        return local[idx] if kind == LOCAL else nxt[idx] if kind == NEXT else F.lift(pub[idx]) if kind == PUBLIC else F.lift(dag.constants[idx]) if kind == CONST else held[idx]
    for at, (what, i) in enumerate(program):
        if what == "emit":
            assert i == len(out)
            out.append(value(dag.dag_constraints[i][1]))
            operands = [dag.dag_constraints[i][1]]
        else:
            op, a, b = dag.nodes[i]
            va, vb = value(a), value(b)
            operands = [a, b]
        for kind, idx in operands:
            if kind == NODE and last[idx] == at:
                held.pop(idx, None)
        if what == "op":
            held[i] = F.mul(va, vb) if op == MUL else F.add(va, vb) if op == ADD else F.sub(va, vb)
            assert len(held) <= max_live
    assert not held
    return out


def _consumer_air(dag):
    """the term-list AIR whose constraint c is the cell num_columns + c of the local row: stark_model's consumer and permutation checks
    then run on a row extended by the DAG's constraint values"""
    return SimpleNamespace(constraints=[(filt, [(1, [(LOCAL, dag.num_columns + c)])]) for c, (filt, _) in enumerate(dag.dag_constraints)], pairs=dag.pairs, q=dag.q)


def eval_vanishing(F, dag, nc, local, nxt, pub, alphas, z_last, l_first, l_last, zs_local=(), zs_next=(), sets=None):
    values = constraint_values(F, dag, local, nxt, pub)
    return sm.eval_vanishing(F, _consumer_air(dag), nc, list(local) + values, nxt, pub, alphas, z_last, l_first, l_last, zs_local, zs_next, sets)


def quotient_values(orc, dag, nc, lg_n, trace_q, zs_q, sets, alphas, pub):
    """stark_model.quotient_values with the DAG's constraints: [nc][n << qdb]"""
    n, size = 1 << lg_n, (1 << lg_n) << dag.qdb
    l_first, l_last = sm.lagrange_on_coset(orc, lg_n, dag.qdb)
    last = pow(primitive_root(lg_n), P - 2, P)
    w = primitive_root(lg_n + dag.qdb)
    rows = np.asarray(trace_q, dtype=U64).T.tolist()
    z_rows = np.asarray(zs_q, dtype=U64).T.tolist() if len(zs_q) else [[]] * size
    out = [[0] * size for _ in range(nc)]
    x = 7
    for i in range(size):
        nx = (i + (1 << dag.qdb)) % size
        accs = eval_vanishing(Base, dag, nc, rows[i], rows[nx], pub, alphas, (x - last) % P, l_first[i], l_last[i], z_rows[i], z_rows[nx], sets)
        z_h_inv = pow((pow(x, n, P) - 1) % P, P - 2, P)
        for j in range(nc):
            out[j][i] = accs[j] * z_h_inv % P
        x = x * w % P
    return out


def vanishing_at(dag, nc, lg_n, zeta, local, nxt, pub, alphas, zs_local=(), zs_next=(), sets=None):
    l_first, l_last = sm.l_first_last_at(lg_n, zeta)
    last = pow(primitive_root(lg_n), P - 2, P)
    return eval_vanishing(sm.Ext, dag, nc, local, nxt, pub, alphas, sm._ext_sub(zeta, (last, 0)), l_first, l_last, zs_local, zs_next, sets)


def verify(dag, nc, params, by, challenger, verify_path, max_queries=None, trace=None):
    """stark_model.verify with the DAG's constraints -> the GL_CHECK_* code of the first failing check"""
    try:
        proof = sm.ParsedStarkProof(dag, nc, params, by)
    except fom.Malformed as e:
        return e.code
    sets, alphas, zeta = sm.replay(dag, nc, proof, challenger)
    if trace is not None:
        trace.update(stark_proof=proof, sets=sets, alphas=alphas, zeta=zeta)
    vanishing = vanishing_at(dag, nc, params.degree_bits, zeta, proof.local, proof.next, proof.public_inputs, alphas, proof.zs, proof.zs_next, sets)
    if not sm.identity_holds(dag, nc, params.degree_bits, zeta, vanishing, proof.quotient):
        return sm.VANISHING
    caps = [proof.trace_cap] + ([proof.zs_cap] if dag.pairs else []) + [proof.quotient_cap]
    return fom.verify(params, sm.fri_instance(dag, nc, zeta, params.degree_bits), np.array(caps, dtype=U64), np.array(proof.fri_openings(), dtype=U64),
                      challenger, proof.fri, verify_path, max_queries=max_queries, trace=trace)


# ------------------------------------------------------------------------------- expansion
class TooManyTerms(Exception):
    pass


def expand(dag, max_terms=MAX_TERMS, zero_columns=()):
    """the DAG multiplied out: constraints as term lists [(filter, [(coeff, [(kind, index), ...]), ...]), ...] with like monomials
    collected and zero coefficients dropped.  Raises TooManyTerms once the constraints expanded so far hold more than max_terms terms.
    zero_columns: LOCAL / NEXT columns set to zero first -- that only removes monomials, so a count under it is a lower bound."""
    polys, total, out = [], 0, []

    def of(o):
        kind, idx = o
        if kind == NODE:
            return polys[idx]
        if kind == CONST:
            return {(): dag.constants[idx] % P} if dag.constants[idx] % P else {}
        return {} if kind in (LOCAL, NEXT) and idx in zero_columns else {((kind, idx),): 1}
    program, _ = schedule(dag)
    needed = {i for what, i in program if what == "op"}
    for k, (op, a, b) in enumerate(dag.nodes):
        if k not in needed:
            polys.append(None)
            continue
        pa, pb = of(a), of(b)
        if op == MUL:
            r = {}
            for ma, ca in pa.items():
                for mb, cb in pb.items():
                    m = tuple(sorted(ma + mb))
                    r[m] = (r.get(m, 0) + ca * cb) % P
        else:
            r = dict(pa)
            for m, c in pb.items():
                r[m] = (r.get(m, 0) + (c if op == ADD else -c)) % P
        polys.append({m: c for m, c in r.items() if c})
    for filt, o in dag.dag_constraints:
        poly = of(o)
        total += len(poly)
        if total > max_terms:
            raise TooManyTerms(total)
        out.append((filt, [(c, list(m)) for m, c in sorted(poly.items())]))
    return out


def expanded_air(dag, **kw):
    """the term-list AIR of stark_airs.py's shape that states the same polynomials"""
    return SimpleNamespace(name=dag.name + "-expanded", num_columns=dag.num_columns, num_public_inputs=dag.num_public_inputs, constraint_degree=dag.constraint_degree,
                           rate_bits=dag.rate_bits, constraints=expand(dag, **kw), pairs=dag.pairs, trace=dag.trace, q=dag.q, qdb=dag.qdb)


# ------------------------------------------------------------------------------- to the library
def word(operand):
    """GL_STARK_OPERAND"""
    return operand[0] << 28 | operand[1]


def desc_of(p, dag):
    """the plonky2_demo_amd.StarkDagDesc of a DAG AIR"""
    return p.StarkDagDesc(dag.num_columns, dag.num_public_inputs, dag.constraint_degree, [(op, word(a), word(b)) for op, a, b in dag.nodes], dag.constants,
                          [(f, word(o)) for f, o in dag.dag_constraints], dag.pairs)
