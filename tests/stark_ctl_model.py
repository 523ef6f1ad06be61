"""A plain Python-integer model of cross-table lookups between STARK tables (no tests here), written from the reference and built on
tests/stark_model.py:
  evm/src/cross_table_lookup.rs:24-116        column_eval          Column::eval / eval_table over either field
  :279-306                                    partial_products     the inclusive running product of one CTL Z
  :178-185, :220-277                          num_ctl_zs, cross_table_lookup_data   a table's CTL Zs, in the reference's order
  :374-414                                    eval_ctl_checks      the two constraints per CTL Z, through the consumer
  :542-569                                    verify_cross_table_lookups
  :596-694                                    check_ctls           the multiset test: "these traces are consistent"
  evm/src/stark.rs:83-142                     fri_instance         the three-batch instance
  plonky2/src/iop/challenger.rs:146-152       CompactChallenger    Challenger::compact on transcript.DuplexChallenger
A system is one of stark_ctl_airs.py: tables (AIRs of stark_airs' shape) and lookups as plain data.  A Column is (terms, constant) with
terms [(trace column, coeff), ...]; a TableWithColumns has .table, .columns and .filter (a Column or None); a lookup is
(looking [TableWithColumns, ...], looked TableWithColumns).
"""
from collections import Counter
from types import SimpleNamespace

import stark_model as sm
from stark_model import Base, P
from transcript import DuplexChallenger
from vanishing_model import primitive_root


class CompactChallenger(DuplexChallenger):
    """transcript.DuplexChallenger with Challenger::compact: duplex if input is pending, clear the output buffer"""

    def compact(self):
        if self.inp:
            self._duplex()
        self.out = []


def poseidon_challenger(orc):
    import numpy as np
    return CompactChallenger(lambda s: orc.poseidon(np.array(s, dtype=np.uint64)), lambda digests: np.asarray(digests, dtype=np.uint64).reshape(-1, 4))


def column_eval(F, column, values):
    """Column::eval: sum_t values[column_t] * coeff_t + constant over the field F (`values` already lifted)"""
    terms, constant = column
    acc = F.zero
    for c, f in terms:
        acc = F.add(acc, F.mul(values[c], F.lift(f)))
    return F.add(acc, F.lift(constant))


def eval_table(column, trace, i):
    """Column::eval_table: on row i of a table given column-major"""
    terms, constant = column
    return (sum(int(trace[c][i]) % P * (f % P) for c, f in terms) + constant) % P


def combine(F, challenge, evals):
    """GrandProductChallenge::combine (evm/src/permutation.rs:61-71): reduce_with_powers(evals, beta) + gamma"""
    beta, gamma = (F.lift(v) for v in challenge)
    acc = F.zero
    for v in reversed(evals):
        acc = F.add(F.mul(acc, beta), v)
    return F.add(acc, gamma)


def partial_products(trace, columns, filter_column, challenge):
    """cross_table_lookup.rs:279-306: Z[i] = prod_{i' <= i} (combine(columns(row i')) if filter(row i') = 1 else 1)"""
    n, acc, out = len(trace[0]), 1, []
    for i in range(n):
        f = eval_table(filter_column, trace, i) if filter_column is not None else 1
        if f == 1:
            acc = acc * combine(Base, challenge, [eval_table(c, trace, i) for c in columns]) % P
        else:
            assert f == 0, "Non-binary filter?"
        out.append(acc)
    return out


def num_ctl_zs(lookups, table, nc):
    return sum(sum(1 for twc in [looked] + list(looking) if twc.table == table) for looking, looked in lookups) * nc


def cross_table_lookup_data(traces, lookups, ctl_challenges):
    """cross_table_lookup.rs:220-277 -> per table the list of its CTL Zs (z values, challenge, columns, filter): lookup by lookup,
    challenge by challenge, the looking tables in order, then the looked one.  A table whose trace is None gets the same list without z."""
    per_table = [[] for _ in range(len(traces))]
    for looking, looked in lookups:
        for challenge in ctl_challenges:
            for twc in list(looking) + [looked]:
                z = partial_products(traces[twc.table], twc.columns, twc.filter, challenge) if traces[twc.table] is not None else None
                per_table[twc.table].append(SimpleNamespace(z=z, challenge=challenge, columns=twc.columns, filter=twc.filter))
    return per_table


def eval_ctl_checks(F, local, nxt, ctl_vars, consume_first_row, consume_transition):
    """eval_cross_table_lookup_checks (cross_table_lookup.rs:374-414); ctl_vars: [(local_z, next_z, CTL Z of cross_table_lookup_data)]"""
    for local_z, next_z, v in ctl_vars:
        def comb(values):
            return combine(F, v.challenge, [column_eval(F, c, values) for c in v.columns])

        def filt(values):
            return column_eval(F, v.filter, values) if v.filter is not None else F.one

        def select(f, x):
            return F.sub(F.add(F.mul(f, x), F.one), f)
        consume_first_row(F.sub(local_z, select(filt(local), comb(local))))
        consume_transition(F.sub(next_z, F.mul(local_z, select(filt(nxt), comb(nxt)))))


def eval_vanishing(F, air, nc, local, nxt, pub, alphas, z_last, l_first, l_last, zs_local, zs_next, sets, ctl_data):
    """evm/src/vanishing_poly.rs: the Stark's constraints, the permutation checks (stark_model.eval_vanishing), then the CTL checks on
    the Zs after the permutation ones (CtlCheckVars::from_proofs skips num_permutation_zs)"""
    nz = sm.num_zs(air, nc)
    accs = sm.eval_vanishing(F, air, nc, local, nxt, pub, alphas, z_last, l_first, l_last, zs_local[:nz], zs_next[:nz], sets)
    lifted = [F.lift(a) for a in alphas]

    def consume(c):
        for j in range(nc):
            accs[j] = F.add(F.mul(accs[j], lifted[j]), c)
    ctl_vars = [(zs_local[nz + k], zs_next[nz + k], v) for k, v in enumerate(ctl_data)]
    eval_ctl_checks(F, local, nxt, ctl_vars, lambda c: consume(F.mul(c, l_first)), lambda c: consume(F.mul(c, z_last)))
    return accs


def verify_cross_table_lookups(lookups, ctl_zs_last, nc):
    """cross_table_lookup.rs:542-569: per lookup and challenge, prod looking Z_last == looked Z_last; ctl_zs_last per table, in order"""
    its = [iter(v) for v in ctl_zs_last]
    ok = True
    for looking, looked in lookups:
        for _ in range(nc):
            prod = 1
            for twc in looking:
                prod = prod * next(its[twc.table]) % P
            ok &= prod == next(its[looked.table])
    assert all(next(it, None) is None for it in its)
    return ok


def check_ctls(traces, lookups):
    """testutils::check_ctls (cross_table_lookup.rs:596-694) -> True iff, per lookup, the filtered looking rows and the filtered looked rows
    are the same multiset"""
    def rows(twc):
        trace, out = traces[twc.table], Counter()
        for i in range(len(trace[0])):
            f = eval_table(twc.filter, trace, i) if twc.filter is not None else 1
            if f == 1:
                out[tuple(eval_table(c, trace, i) for c in twc.columns)] += 1
            else:
                assert f == 0, "Non-binary filter?"
        return out
    return all(sum((rows(t) for t in looking), Counter()) == rows(looked) for looking, looked in lookups)


def fri_instance(air, nc, nctl, zeta, lg_n):
    """evm/src/stark.rs:83-142 as fri_openings_model takes it: oracles trace, Z (permutation then CTL), quotient; a third batch at g^-1
    with the CTL Zs only"""
    nz, g = sm.num_zs(air, nc), primitive_root(lg_n)
    oracles = [(air.num_columns, False), (nz + nctl, False), (air.q * nc, False)]
    trace = [(0, c) for c in range(air.num_columns)]
    zs = [(1, c) for c in range(nz + nctl)]
    quotient = [(2, c) for c in range(air.q * nc)]
    zeta = (int(zeta[0]) % P, int(zeta[1]) % P)
    batches = [(zeta, trace + zs + quotient), ((zeta[0] * g % P, zeta[1] * g % P), trace + zs)]
    if nctl:
        batches.append(((pow(g, P - 2, P), 0), [(1, nz + c) for c in range(nctl)]))
    return SimpleNamespace(oracles=oracles, batches=batches)


def quotient_values(orc, air, nc, lg_n, trace_q, zs_q, sets, alphas, pub, ctl_data):
    """compute_quotient_polys (evm/src/prover.rs:469-600) before its coset_ifft, as stark_model.quotient_values with the CTL checks:
    trace_q [num_columns][size], zs_q [nz + nctl][size] = the LDE values at the points 7 w^i of the quotient coset -> [nc][size]"""
    import numpy as np
    n, size = 1 << lg_n, (1 << lg_n) << air.qdb
    l_first, l_last = sm.lagrange_on_coset(orc, lg_n, air.qdb)
    last = pow(primitive_root(lg_n), P - 2, P)
    w = primitive_root(lg_n + air.qdb)
    rows = np.asarray(trace_q, dtype=np.uint64).T.tolist()
    z_rows = np.asarray(zs_q, dtype=np.uint64).T.tolist()
    out = [[0] * size for _ in range(nc)]
    x = 7
    for i in range(size):
        nx = (i + (1 << air.qdb)) % size
        accs = eval_vanishing(Base, air, nc, rows[i], rows[nx], pub, alphas, (x - last) % P, l_first[i], l_last[i], z_rows[i], z_rows[nx], sets, ctl_data)
        z_h_inv = pow((pow(x, n, P) - 1) % P, P - 2, P)
        for j in range(nc):
            out[j][i] = accs[j] * z_h_inv % P
        x = x * w % P
    return out


# ------------------------------------------------------------------------------- the set proof's bytes, the transcript and the model verifier
CTL = 14                                                              # GL_CHECK_CTL


class ParsedTableProof(sm.ParsedStarkProof):
    """One table's proof in the set layout of include/plonky2_mi355x.h: as stark_model.ParsedStarkProof with the Z cap always present and
    ctl_zs_last[nctl] (one word each) between permutation_ctl_zs_next and quotient_polys"""

    def __init__(self, air, nc, nctl, params, by):
        import fri_openings_model as fom
        self.by, self.pos, self.keccak = bytes(by), 0, bool(params.hasher)
        nzs, ncap = sm.num_zs(air, nc) + nctl, 1 << params.cap_height
        self.trace_cap, self.zs_cap, self.quotient_cap = self.hashes(ncap), self.hashes(ncap), self.hashes(ncap)
        self.local, self.next = self.exts(air.num_columns), self.exts(air.num_columns)
        self.zs, self.zs_next = self.exts(nzs), self.exts(nzs)
        self.ctl_zs_last = self.words(nctl)
        self.quotient = self.exts(air.q * nc)
        self.fri = self.take(sm.fri_proof_size(params, fri_instance(air, nc, nctl, (0, 1), params.degree_bits)))
        self.public_inputs = self.words(air.num_public_inputs)
        if self.pos != len(self.by):
            raise fom.Malformed(fom.LENGTH)

    def fri_openings(self):
        """to_fri_openings (evm/src/proof.rs:261-292): [local, zs, quotient], [next, zs_next], [ctl_zs_last lifted to the extension]"""
        return self.local + self.zs + self.quotient + self.next + self.zs_next + [(v, 0) for v in self.ctl_zs_last]


def table_proof_size(air, nc, nctl, params):
    hb = 25 if params.hasher else 32
    return (3 * (hb << params.cap_height) + 16 * (2 * air.num_columns + 2 * (sm.num_zs(air, nc) + nctl) + air.q * nc) + 8 * nctl +
            sm.fri_proof_size(params, fri_instance(air, nc, nctl, (0, 1), params.degree_bits)) + 8 * air.num_public_inputs)


def split_set_proof(tables, lookups, nc, params, by):
    """the set proof = the tables' proofs one after the other, every size fixed by the description -> [ParsedTableProof], or a code"""
    import fri_openings_model as fom
    nctl = [num_ctl_zs(lookups, t, nc) for t in range(len(tables))]
    sizes = [table_proof_size(a, nc, k, p) for a, k, p in zip(tables, nctl, params)]
    if len(by) < sum(sizes):
        raise fom.Malformed(fom.TRUNCATED)
    if len(by) > sum(sizes):
        raise fom.Malformed(fom.LENGTH)
    out, pos = [], 0
    for a, k, p, size in zip(tables, nctl, params, sizes):
        out.append(ParsedTableProof(a, nc, k, p, by[pos:pos + size]))
        pos += size
    return out


def verify_set(tables, lookups, nc, params, by, challenger, verify_path, max_queries=None, trace=None):
    """verify_proof (evm/src/verifier.rs:29-216) in the order gl_stark_set_verify documents -> (GL_CHECK_* code, table): the trace caps and
    the CTL challenges (get_challenges.rs:18-49); per table compact, its challenges, the vanishing identity at zeta over the extension with
    the CTL checks, the three-batch FRI checks; last verify_cross_table_lookups.  `challenger` has compact (CompactChallenger)."""
    import numpy as np

    import fri_openings_model as fom
    T = len(tables)
    try:
        proofs = split_set_proof(tables, lookups, nc, params, by)
    except fom.Malformed as e:
        return e.code, T
    for pr in proofs:
        challenger.observe_hashes(np.array(pr.trace_cap, dtype=np.uint64))
    ctl_challenges = [tuple(challenger.get(2)) for _ in range(nc)]
    data = cross_table_lookup_data([None] * T, lookups, ctl_challenges)
    if trace is not None:
        trace.update(ctl_challenges=ctl_challenges, tables=[])
    for t, (air, p, pr) in enumerate(zip(tables, params, proofs)):
        challenger.compact()
        sets = [[tuple(challenger.get(2)) for _ in range(nc)] for _ in range(air.q)] if air.pairs else None
        challenger.observe_hashes(np.array(pr.zs_cap, dtype=np.uint64))
        alphas = challenger.get(nc)
        challenger.observe_hashes(np.array(pr.quotient_cap, dtype=np.uint64))
        zeta = tuple(challenger.get(2))
        challenger.observe(np.array(pr.fri_openings(), dtype=np.uint64))
        sub = {} if trace is not None else None
        if trace is not None:
            sub.update(table_proof=pr, sets=sets, alphas=alphas, zeta=zeta)         # fri_openings_model.verify adds its own keys (proof: the FriProof)
            trace["tables"].append(sub)
        l_first, l_last = sm.l_first_last_at(p.degree_bits, zeta)
        last = pow(primitive_root(p.degree_bits), P - 2, P)
        accs = eval_vanishing(sm.Ext, air, nc, pr.local, pr.next, pr.public_inputs, alphas, sm._ext_sub(zeta, (last, 0)), l_first, l_last, pr.zs, pr.zs_next,
                              sets, data[t])
        if not sm.identity_holds(air, nc, p.degree_bits, zeta, accs, pr.quotient):
            return sm.VANISHING, t
        caps = [pr.trace_cap, pr.zs_cap, pr.quotient_cap]
        code = fom.verify(p, fri_instance(air, nc, len(data[t]), zeta, p.degree_bits), np.array(caps, dtype=np.uint64), np.array(pr.fri_openings(), dtype=np.uint64),
                          challenger, pr.fri, verify_path, max_queries=max_queries, trace=sub)
        if code:
            return code, t
    if not verify_cross_table_lookups(lookups, [pr.ctl_zs_last for pr in proofs], nc):
        return CTL, T
    return 0, T
