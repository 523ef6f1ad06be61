"""CPU tests of the DAG model tests/stark_dag_model.py and of the AIRs of tests/stark_dag_airs.py: the model against stark_model on the
expansion of every AIR small enough to expand, the scheduling and liveness definition on cases counted by hand, the quotient of a
satisfying trace under trim_to_len(q n) with the bound cases on the bound, and plonky2_demo_amd.StarkDagBuilder against the model's."""
import numpy as np
import pytest

import stark_airs
import stark_dag_airs as da
import stark_dag_model as dm
import stark_model as sm
from stark_airs import ALL, FIRST_ROW, LAST_ROW, P, TRANSITION

U64 = np.uint64
EXPANDABLE = [name for name in da.EVERY if name != "sbox2"]


def random_row(rng, k):
    return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]


@pytest.mark.parametrize("name", EXPANDABLE)
def test_the_model_equals_stark_model_on_the_expansion(name):
    dag = da.EVERY[name]
    dm.check(dag)
    expanded = dm.expanded_air(dag)
    rng = np.random.Generator(np.random.PCG64(41))
    for _ in range(3):
        local, nxt, pub = random_row(rng, dag.num_columns), random_row(rng, dag.num_columns), random_row(rng, dag.num_public_inputs)
        want = sm.constraint_values(sm.Base, expanded, local, nxt, pub)
        assert dm.constraint_values(sm.Base, dag, local, nxt, pub) == want
        if name in stark_airs.AIRS:                                      # the converted ones: the term list they came from, too
            assert sm.constraint_values(sm.Base, stark_airs.AIRS[name], local, nxt, pub) == want
        le, ne = [(v, w) for v, w in zip(local, random_row(rng, dag.num_columns))], [(v, w) for v, w in zip(nxt, random_row(rng, dag.num_columns))]
        assert dm.constraint_values(sm.Ext, dag, le, ne, pub) == sm.constraint_values(sm.Ext, expanded, le, ne, pub)
    # the whole consumer, permutation checks included, on one row
    nc = 3
    alphas, zs, zn = random_row(rng, nc), random_row(rng, sm.num_zs(dag, nc)), random_row(rng, sm.num_zs(dag, nc))
    sets = [[tuple(random_row(rng, 2)) for _ in range(nc)] for _ in range(dag.q)]
    args = (nc, local, nxt, pub, alphas, 5, 6, 7, zs, zn, sets)
    assert dm.eval_vanishing(sm.Base, dag, *args) == sm.eval_vanishing(sm.Base, expanded, *args)
    assert [f for f, _ in expanded.constraints] == [f for f, _ in dag.dag_constraints]


def test_the_expansion_of_sbox2_passes_the_term_cap_and_that_of_every_other_air_does_not():
    # 12 transition constraints of 7832 monomials each (1 + 108 + 1782 + 5940 products of at most three x_j^e, plus the next cell)
    with pytest.raises(dm.TooManyTerms) as e:
        dm.expand(da.sbox2)
    assert e.value.args[0] > dm.MAX_TERMS == 65536
    out = dm.expand(da.sbox2, max_terms=1 << 30)
    assert [len(t) for _, t in out] == [2] * 12 + [7832] * 12 + [2] and sum(len(t) for _, t in out) == 94010
    for name in EXPANDABLE:
        assert sum(len(t) for _, t in dm.expand(da.EVERY[name])) <= dm.MAX_TERMS
    assert max(dm.degrees(da.sbox2)[1]) == 9 == da.sbox2.q + 1 and da.sbox2.rate_bits == 3


def test_degrees_schedules_and_live_counts_counted_by_hand():
    b = dm.Builder(3, 1)
    x, y, z = b.local(0), b.local(1), b.next(2)
    late = x * y                                     # node 0, behind constraint 2
    dead = late * z                                  # node 1, never used
    first = x + b.public(0)                          # node 2, behind constraint 1
    b.constraint_first_row(b.public(0))              # constraint 0: a bare operand, consumed before node 0
    b.constraint(first)
    b.constraint_transition(late - z)                # node 3
    b.constraint(first * first)                      # node 4: first dies into it
    assert dead.operand == (dm.NODE, 1)
    dag = dm.dag_air("hand", 3, 1, 3, 1, b, [], None)
    assert dm.degrees(dag) == ([2, 3, 1, 2, 2], [0, 1, 2, 2])
    program, max_live = dm.schedule(dag)
    assert program == [("emit", 0), ("op", 0), ("op", 2), ("emit", 1), ("op", 3), ("emit", 2), ("op", 4), ("emit", 3)]
    assert max_live == 2                             # late and first; late dies into node 3, first into node 4
    # the AIRs' own
    assert dm.schedule(da.at_cap())[1] == 128 == dm.MAX_LIVE and dm.schedule(da.at_cap(129))[1] == 129
    with pytest.raises(dm.Refused, match="live"):
        dm.check(da.at_cap(129))
    assert dm.schedule(da.alias)[1] == 4             # keep, t, u and the chain that runs beside them
    program, _ = dm.schedule(da.operands)
    assert len(program) == len(da.operands.nodes) - 2 + len(da.operands.dag_constraints)       # the two dead nodes are dropped
    emitted = [i for what, i in program if what == "emit"]
    assert emitted == list(range(len(da.operands.dag_constraints)))                            # the yield order, whatever the nodes' order
    late_node = da.operands.dag_constraints[-1][1][1]
    assert late_node < da.operands.dag_constraints[0][1][1]                                    # defined first, consumed last
    for name, dag in da.BOUND.items():
        (filt, _), = dag.dag_constraints
        assert dm.degrees(dag)[1] == [dag.q if filt in (FIRST_ROW, LAST_ROW) else dag.q + 1], name
    assert sorted(d.q for d in da.BOUND.values()) == [1] * 4 + [3] * 4 + [8] * 4


def test_every_rule_of_the_model_refuses_one_step_beyond():
    def dag(nodes, constraints, constants=(5,), degree=3, columns=2, pis=1):
        b = dm.Builder(columns, pis)
        b.nodes, b.constants, b.constraints = list(nodes), list(constants), list(constraints)
        return dm.dag_air("rule", columns, pis, degree, 1, b, [], None)
    L0, K0 = (dm.LOCAL, 0), (dm.CONST, 0)
    ok = dag([(dm.MUL, L0, L0), (dm.MUL, (dm.NODE, 0), L0)], [(ALL, (dm.NODE, 1))])
    dm.check(ok)
    for what, bad in [("no earlier node", dag([(dm.ADD, (dm.NODE, 0), L0)], [(ALL, (dm.NODE, 0))])),
                      ("no earlier node", dag([(dm.ADD, L0, (dm.NODE, 1)), (dm.ADD, L0, L0)], [(ALL, (dm.NODE, 0))])),
                      ("op", dag([(3, L0, L0)], [(ALL, (dm.NODE, 0))])),
                      ("operand kind", dag([(dm.ADD, (5, 0), L0)], [(ALL, (dm.NODE, 0))])),
                      ("index out of range", dag([(dm.ADD, (dm.LOCAL, 2), L0)], [(ALL, (dm.NODE, 0))])),
                      ("index out of range", dag([(dm.ADD, (dm.CONST, 1), L0)], [(ALL, (dm.NODE, 0))])),
                      ("index out of range", dag([], [(ALL, (dm.NODE, 0))])),
                      ("filter", dag([], [(4, K0)])),
                      ("count", dag([], [])),
                      ("degree", dag([(dm.MUL, L0, L0), (dm.MUL, (dm.NODE, 0), (dm.NODE, 0))], [(ALL, (dm.NODE, 1))])),
                      ("degree", dag([(dm.MUL, L0, L0), (dm.MUL, (dm.NODE, 0), L0)], [(FIRST_ROW, (dm.NODE, 1))]))]:
        with pytest.raises(dm.Refused, match=what):
            dm.check(bad)


# ------------------------------------------------------------------------------- the quotient of a satisfying trace
def quotient_coefficients(orc, dag, nc, lg_n, seed=3):
    trace, pis = dag.trace(1 << lg_n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(77))
    sets = [[tuple(random_row(rng, 2)) for _ in range(nc)] for _ in range(dag.q)]
    alphas = random_row(rng, nc)
    coeffs = orc.ifft(trace)
    zs = sm.permutation_zs(dag, nc, trace, sets)[0] if dag.pairs else []
    zs_q = orc.lde(orc.ifft(np.array(zs, dtype=U64)), dag.qdb) if zs else []
    values = dm.quotient_values(orc, dag, nc, lg_n, orc.lde(coeffs, dag.qdb), zs_q, sets, alphas, pis)
    return orc.coset_ifft(np.array(values, dtype=U64), 7)


@pytest.mark.parametrize("name", list(da.OWN))
def test_the_quotient_of_a_satisfying_trace_passes_the_trim(orc, name):
    dag, lg_n = da.OWN[name], 4 if name.startswith("at_cap") else 5
    n = 1 << lg_n
    coeffs = quotient_coefficients(orc, dag, 1, lg_n)
    assert coeffs.shape == (1, n << dag.qdb)
    assert not coeffs[:, dag.q * n:].any(), "trim_to_len(q n) fails on a satisfying trace"
    if name in da.BOUND:
        # exactly on the bound: C has degree d (n - 1), the filter adds n - 1 (1 under TRANSITION, nothing under ALL), Z_H takes n.  One
        # trace factor more would add n - 1 and pass q n.
        (filt, _), = dag.dag_constraints
        d = dag.q if filt in (FIRST_ROW, LAST_ROW) else dag.q + 1
        top = d * (n - 1) + {ALL: 0, TRANSITION: 1, FIRST_ROW: n - 1, LAST_ROW: n - 1}[filt] - n
        assert dag.q * n - (n - 1) <= top + 1 <= dag.q * n
        assert coeffs[0, top] != 0 and not coeffs[0, top + 1:].any(), "the quotient's top coefficient is not where the bound puts it"


def test_a_broken_cell_fails_the_trim_where_q_is_no_power_of_two(orc):
    dag = da.BOUND["bound-constraint_transition-q3"]
    trace, pis = dag.trace(32, seed=3)
    bad = dag.trace

    def broken(n, seed=0):
        t, p = bad(n, seed)
        t = t.copy()
        t[0, 9] = (int(t[0, 9]) + 1) % P
        return t, p
    dag_bad = type(dag)(**{**vars(dag), "trace": broken})
    assert quotient_coefficients(orc, dag_bad, 1, 5)[:, dag.q * 32:].any()


# ------------------------------------------------------------------------------- the library's builder
@pytest.mark.parametrize("write,columns,pis", [(da.write_sbox2, da.WIDTH, da.WIDTH + 1), (da.write_alias, 4, 0), (da.write_operands, da.OPERANDS_COLUMNS, 2),
                                               (da.write_at_cap(5), 3, 0), (lambda b: da.write_terms(b, stark_airs.quartic), 9, 3)],
                         ids=["sbox2", "alias", "operands", "at_cap5", "quartic"])
def test_the_librarys_builder_writes_what_the_models_builder_writes(write, columns, pis):
    import plonky2_demo_amd as p
    mine, theirs = dm.Builder(columns, pis), p.StarkDagBuilder(columns, pis)
    write(mine)
    write(theirs)
    desc = theirs.build(3)
    assert isinstance(desc, p.StarkDagDesc) and isinstance(desc, p.StarkDesc) and desc.constraints == []
    assert desc.nodes == [(op, dm.word(a), dm.word(b)) for op, a, b in mine.nodes]
    assert desc.constants == mine.constants and desc.dag_constraints == [(f, dm.word(o)) for f, o in mine.constraints]


def test_the_builder_is_hash_consed_and_coerces_ints():
    import plonky2_demo_amd as p
    b = p.StarkDagBuilder(2, 1)
    x, y = b.local(0), b.next(1)
    assert (x * y + 3).word == (x * y + 3).word and len(b.nodes) == 2 and b.constants == [3]       # written twice: one node each, one constant
    assert (3 + x * y).word != (x * y + 3).word and len(b.nodes) == 3                                # no rewriting: the operand order is the writer's
    assert (x - 1).word != (1 - x).word and b.constants == [3, 1]
    assert b.const(-1).word == b.const(P - 1).word and b.const(P).word != b.const(0).word         # a 64-bit word stands as it is
    assert b.const(2**64 - 1).word != b.const((2**64 - 1) % P).word
    b.constraint_first_row(x - b.public(0))
    b.constraint(5)
    assert [f for f, _ in b.constraints] == [p.GL_STARK_FIRST_ROW, p.GL_STARK_ALL]
    with pytest.raises(ValueError):
        x + p.StarkDagBuilder(2, 1).local(0)
