"""CPU tests that pin the model tests/stark_ctl_model.py on the system of tests/stark_ctl_airs.py: the model is what the GPU tests of
tests/test_stark_ctl.py compare the device against."""
import copy

import numpy as np
import pytest

import stark_ctl_airs as airs
import stark_ctl_model as cm
import stark_model as sm
from stark_model import Base, Ext, P

U64 = np.uint64
LGS = [5, 6, 5]


def challenges(rng, nc):
    return [tuple(int(v) for v in rng.integers(0, P, size=2, dtype=U64)) for _ in range(nc)]


def lasts(traces, lookups, chs):
    return [[v.z[-1] for v in zs] for zs in cm.cross_table_lookup_data(traces, lookups, chs)]


def test_column_eval_is_the_linear_combination_over_both_fields():
    col = ([(0, 3), (2, P + 5)], 2**64 - 1)                               # non-canonical coefficient and constant
    row = [7, 11, P - 1]
    want = (3 * 7 + 5 * (P - 1) + (2**64 - 1)) % P
    assert cm.column_eval(Base, col, row) == want
    assert cm.column_eval(Ext, col, [(v, 0) for v in row]) == (want, 0)
    assert cm.eval_table(col, [[v] for v in row], 0) == want
    assert cm.column_eval(Base, ([], 9), row) == 9                        # an empty combination is a constant
    assert cm.column_eval(Ext, col, [(7, 1), (0, 0), (0, 2)]) == ((3 * 7 + 2**64 - 1) % P, (3 + 5 * 2) % P)


def test_partial_products_is_inclusive_and_skips_filtered_rows():
    trace = [[2, 3, 5, 7], [1, 0, 1, 1]]
    z = cm.partial_products(trace, [cm_single(0)], cm_single(1), (10, 100))
    assert z == [102, 102, 102 * 105, 102 * 105 * 107]                    # Z[0] holds row 0's factor: inclusive
    assert cm.partial_products(trace, [cm_single(0)], None, (10, 100)) == [102, 102 * 103, 102 * 103 * 105, 102 * 103 * 105 * 107]
    two = cm.partial_products(trace, [cm_single(0), cm_single(1)], None, (10, 100))
    assert two[0] == 2 + 10 * 1 + 100                                     # reduce_with_powers: sum beta^k column_k, then + gamma
    with pytest.raises(AssertionError, match="Non-binary"):
        cm.partial_products([[1], [2]], [cm_single(0)], cm_single(1), (1, 1))


def cm_single(c):
    return airs.single(c)


@pytest.mark.parametrize("nc", [1, 2])
def test_ctl_zs_are_in_the_reference_s_order(nc):
    # cross_table_lookup_data (cross_table_lookup.rs:220-277): lookup by lookup, challenge by challenge, looking tables, then the looked
    chs = [(j + 1, j + 50) for j in range(nc)]
    data = cm.cross_table_lookup_data([None] * 3, airs.LOOKUPS, chs)
    (look0, look0b), looked0 = airs.LOOKUPS[0]
    (look1,), looked1 = airs.LOOKUPS[1]
    assert [(v.challenge, v.columns) for v in data[airs.OPS]] == [(c, look0.columns) for c in chs] + [(c, looked1.columns) for c in chs]
    assert [(v.challenge, v.columns) for v in data[airs.OPS2]] == [(c, look0b.columns) for c in chs]
    assert [(v.challenge, v.columns) for v in data[airs.MUL]] == [(c, looked0.columns) for c in chs] + [(c, look1.columns) for c in chs]
    assert [len(d) for d in data] == [cm.num_ctl_zs(airs.LOOKUPS, t, nc) for t in range(3)]


def test_last_values_multiply_out_exactly_when_check_ctls_accepts():
    rng = np.random.Generator(np.random.PCG64(11))
    chs = challenges(rng, 2)
    good = airs.traces(LGS, seed=2)
    assert cm.check_ctls(good, airs.LOOKUPS)
    assert cm.verify_cross_table_lookups(airs.LOOKUPS, lasts(good, airs.LOOKUPS, chs), 2)
    removed = airs.remove_one_looked_row(good)
    assert not cm.check_ctls(removed, airs.LOOKUPS)
    assert not cm.verify_cross_table_lookups(airs.LOOKUPS, lasts(removed, airs.LOOKUPS, chs), 2)
    # one changed looked cell breaks both (lookup 1: ops' w on one row)
    changed = [t.copy() for t in good]
    changed[airs.OPS][6][9] = (int(changed[airs.OPS][6][9]) + 1) % P
    assert not cm.check_ctls(changed, airs.LOOKUPS)
    assert not cm.verify_cross_table_lookups(airs.LOOKUPS, lasts(changed, airs.LOOKUPS, chs), 2)
    # each lookup is judged on its own: lookup 0 of `changed` still holds
    assert cm.check_ctls(changed, airs.LOOKUPS[:1])


@pytest.mark.parametrize("nc", [1, 2])
def test_the_quotient_of_a_consistent_system_has_degree_below_q_n(orc, nc):
    # every table: the values of (sum alpha^i C_i) / Z_H on the quotient coset interpolate to a polynomial that passes trim_to_len(q n)
    # (evm/src/prover.rs:392-396).  The longest CTL term, Z(x) f(g x) combine(g x) (x - g^-1) / Z_H, has degree 3 (n - 1) + 1 - n = 2 n - 2:
    # the top coefficient the trim keeps at q = 2 is non-zero, so the term sits exactly on the bound.  At q = 2 the quotient coset has
    # exactly q n points and the trim nothing to cut, so the values are taken on a coset of 4 n points here, where the trim has a tail
    rng = np.random.Generator(np.random.PCG64(12 + nc))
    traces = airs.traces(LGS, seed=3)
    chs = challenges(rng, nc)
    data = cm.cross_table_lookup_data(traces, airs.LOOKUPS, chs)
    for table, air in enumerate(airs.TABLES):
        lg_n = LGS[table]
        n = 1 << lg_n
        air = copy.copy(air)
        air.qdb = 2
        sets = [[tuple(int(v) for v in rng.integers(0, P, size=2, dtype=U64)) for _ in range(nc)] for _ in range(air.q)] if air.pairs else None
        zs = (sm.permutation_zs(air, nc, traces[table], sets)[0] if air.pairs else []) + [v.z for v in data[table]]
        trace_q = orc.lde(orc.ifft(traces[table]), air.qdb)
        zs_q = orc.lde(orc.ifft(np.array(zs, dtype=U64)), air.qdb)
        alphas = [int(v) for v in rng.integers(0, P, size=nc, dtype=U64)]
        values = cm.quotient_values(orc, air, nc, lg_n, trace_q, zs_q, sets, alphas, [], data[table])
        coeffs = orc.coset_ifft(np.array(values, dtype=U64), 7)
        assert not coeffs[:, air.q * n:].any(), "table %d: the quotient's degree is too high" % table
        assert coeffs.shape[1] == 4 * n and coeffs[:, air.q * n - 2].all() and not coeffs[:, air.q * n - 1].any()
        # and a Z that breaks the running product does not pass
        zs_bad = np.array(zs, dtype=U64)
        zs_bad[-1][n // 2] = (int(zs_bad[-1][n // 2]) + 1) % P
        bad = cm.quotient_values(orc, air, nc, lg_n, trace_q, orc.lde(orc.ifft(zs_bad), air.qdb), sets, alphas, [], data[table])
        assert orc.coset_ifft(np.array(bad, dtype=U64), 7)[:, air.q * n:].any()


@pytest.mark.parametrize("nc", [1, 2, 3, 4])
def test_the_quotient_of_the_system_with_a_degree_5_table_has_degree_below_q_n(orc, nc):
    # TABLES5: the same traces satisfy it (used^5 = used); ops and ops2 keep q = 2, mul has q = 4.  Every table on a coset twice as large
    # as its own, so that the trim has a tail to look at; mul's own constraint used^5 - used sits on the bound: degree 5 (n - 1) - n
    rng = np.random.Generator(np.random.PCG64(40 + nc))
    traces = airs.traces(LGS, seed=3)
    chs = challenges(rng, nc)
    data = cm.cross_table_lookup_data(traces, airs.LOOKUPS, chs)
    assert [(a.q, a.qdb, a.rate_bits) for a in airs.TABLES5] == [(2, 1, 2), (2, 1, 2), (4, 2, 2)]
    assert [len(d) for d in data] == [cm.num_ctl_zs(airs.LOOKUPS, t, nc) for t in range(3)] == [2 * nc, nc, 2 * nc]
    for table, air in enumerate(airs.TABLES5):
        lg_n = LGS[table]
        n = 1 << lg_n
        air = copy.copy(air)
        air.qdb += 1
        sets = [[tuple(int(v) for v in rng.integers(0, P, size=2, dtype=U64)) for _ in range(nc)] for _ in range(air.q)] if air.pairs else None
        zs = (sm.permutation_zs(air, nc, traces[table], sets)[0] if air.pairs else []) + [v.z for v in data[table]]
        trace_q = orc.lde(orc.ifft(traces[table]), air.qdb)
        zs_q = orc.lde(orc.ifft(np.array(zs, dtype=U64)), air.qdb)
        alphas = [int(v) for v in rng.integers(0, P, size=nc, dtype=U64)]
        values = cm.quotient_values(orc, air, nc, lg_n, trace_q, zs_q, sets, alphas, [], data[table])
        coeffs = orc.coset_ifft(np.array(values, dtype=U64), 7)
        assert coeffs.shape == (nc, 2 * n << (air.qdb - 1)) and not coeffs[:, air.q * n:].any(), "table %d: the quotient's degree is too high" % table
        if table == airs.MUL:
            assert coeffs[:, 4 * n - 5].all() and not coeffs[:, 4 * n - 4:].any()
        zs_bad = np.array(zs, dtype=U64)
        zs_bad[-1][n // 2] = (int(zs_bad[-1][n // 2]) + 1) % P
        bad = cm.quotient_values(orc, air, nc, lg_n, trace_q, orc.lde(orc.ifft(zs_bad), air.qdb), sets, alphas, [], data[table])
        assert orc.coset_ifft(np.array(bad, dtype=U64), 7)[:, air.q * n:].any()
        # a row with used = 2 satisfies used (a b - c) = 0 where a b = c, but not used^5 = used
        if table == airs.MUL:
            broken = traces[table].copy()
            broken[3][int(np.flatnonzero(broken[3])[0])] = 2
            values = cm.quotient_values(orc, air, nc, lg_n, orc.lde(orc.ifft(broken), air.qdb), zs_q, sets, [0] * (nc - 1) + [1], [], [])
            assert orc.coset_ifft(np.array(values, dtype=U64), 7)[:, air.q * n:].any()


def test_compact_against_a_hand_run_of_the_duplex_sponge(orc):
    # challenger.rs:146-152 by hand on the permutation: pending input is written over the first words of the state and permuted; the
    # outputs are dropped, so the next challenge permutes again
    perm = lambda s: [int(x) for x in orc.poseidon(np.array(s, dtype=U64))]      # noqa: E731
    ch = cm.poseidon_challenger(orc)
    ch.observe([5, 6, 7])
    ch.compact()
    s1 = perm([5, 6, 7] + [0] * 9)
    assert ch.state == s1 and ch.inp == [] and ch.out == []
    s2 = perm(s1)
    assert ch.get(2) == [s2[7] % P, s2[6] % P]                            # nothing pending: a fresh permutation, popped from the end of the rate
    ch.compact()                                                          # outputs only: dropped without a permutation
    assert ch.state == s2 and ch.out == []
    s3 = perm(s2)
    assert ch.get(1) == [s3[7] % P]
    # without compact the same draws come from one permutation
    plain = cm.poseidon_challenger(orc)
    plain.observe([5, 6, 7])
    assert plain.get(3) == [s1[7] % P, s1[6] % P, s1[5] % P]


def test_the_instance_has_a_third_batch_with_the_ctl_zs_only():
    inst = cm.fri_instance(airs.ops2, 2, 2, (3, 4), 6)
    g = sm.primitive_root(6)
    assert inst.oracles == [(7, False), (1 + 2, False), (2 * 2, False)]
    assert [len(polys) for _, polys in inst.batches] == [7 + 3 + 4, 7 + 3, 2]
    assert inst.batches[2] == ((pow(g, P - 2, P), 0), [(1, 1), (1, 2)])   # g^-1 in the base field; the permutation Z (index 0) is not opened there
    assert inst.batches[1][0] == (3 * g % P, 4 * g % P)
    assert len(cm.fri_instance(airs.ops2, 2, 0, (3, 4), 6).batches) == 2  # no CTL Z: the single-table instance
