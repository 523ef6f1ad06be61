"""The Python-integer model of the sigma polynomials (tests/sigma_model.py) on its own evidence, before it judges a kernel
(tests/test_sigma.py), and a guard on the crafted partitions that test uses (tests/sigma_cases.py).  CPU only.

Against the oracle: the oracle builds its circuits with the generic builder and a union-find forest.  Its sigma columns, decoded into a
partition by following cycles and pushed through the model, come back word for word: the cycles walk their wires in (row, column) order, as
the model (and the reference's wire_partition) does.  Against the host: the closed-form sigma columns of the matmul family, plain and
zero-knowledge, are the model on the host's wire classes.  Against the ext-gate builder: the model's sigma is a permutation of the wires
whose cycles are the builder's union-find sets."""
import ctypes

import numpy as np
import pytest

import ext_gate_circuits as egc
import sigma_cases as sc
import sigma_model as sm

U64 = np.uint64
MATMULS = [1, 2, 3, 5, 8]
# (kind, param): the gates beyond Noop / Constant / PublicInput / Arithmetic that the oracle circuit has
ORACLE_KINDS = {
    (15, 1): "PoseidonGate, BaseSumGate, ExponentiationGate, two lookup tables",
    (16, 3): "RandomAccessGate",
    (17, 3): "PoseidonGate, RandomAccessGate, BaseSumGate (Merkle proof to a cap)",
    (14, 3): "PoseidonGate, BaseSumGate (Merkle proof)",
    (2, 50): "ArithmeticGate alone, no public inputs",
}


def k_is_of(d):
    return [int(d.k_is[j]) for j in range(80)]


def oracle_circuit(orc, key):
    return orc.circuit(key, threads=4) if isinstance(key, int) else orc.circuit_of_kind(key[0], key[1], threads=4)


# ------------------------------------------------------------------------------- the model against the oracle's forest
@pytest.mark.parametrize("key", MATMULS + list(ORACLE_KINDS), ids=lambda k: "matmul m = %d" % k if isinstance(k, int) else "kind %d (%d)" % k)
def test_decode_then_model_reproduces_the_oracle_sigma_columns(orc, key):
    oc = oracle_circuit(orc, key)
    d = oc.product_desc()
    lg_n, k_is = d.degree_bits, k_is_of(d)
    want = oc.constants_sigmas()[d.num_constants:]
    classes = sm.classes_from_sigma(want, k_is, lg_n)
    got = np.array(sm.sigma_values(classes, k_is, lg_n), dtype=U64)
    assert (got == want).all(), "%d of %d sigma values differ" % ((got != want).sum(), want.size)
    sizes = [len(s) for s in sm.wire_partition(classes, lg_n).values()]
    assert max(sizes) > 2 and sizes.count(1) > len(sizes) // 2         # a real partition: mostly singletons, some larger classes
    # the decoding itself: a class id is the first wire of its class, and relabelling the classes changes nothing
    first = {}
    for row in range(1 << lg_n):
        for col in range(80):
            first.setdefault(classes[col][row], row * 80 + col)
    assert all(ident == q for ident, q in first.items())
    relabelled = sc.high_word_relabel(np.array(classes, dtype=U64))
    assert (np.array(sm.sigma_values(relabelled, k_is, lg_n), dtype=U64) == want).all()


# ------------------------------------------------------------------------------- the model against the host's closed form
@pytest.mark.parametrize("zk", [False, True], ids=["plain", "zero-knowledge"])
@pytest.mark.parametrize("m", MATMULS)
def test_model_on_the_host_classes_is_the_host_closed_form(m, zk):
    # host-only entries: no GPU.  The zero-knowledge builds are circuits the oracle cannot construct.
    import plonky2_demo_amd as p
    from plonky2_demo_amd._lib import check, lib
    hc = p.MatmulCircuit(m, zero_knowledge=zk)
    d = hc.desc
    classes = np.empty((80, hc.n), dtype=U64)
    check(lib.gl_host_circuit_wire_classes(hc.handle, classes.ctypes.data_as(ctypes.c_void_p)))
    want = hc.constants_sigmas()[d.num_constants:]
    got = np.array(sm.sigma_values(classes, k_is_of(d), d.degree_bits), dtype=U64)
    assert (got == want).all(), "%d of %d sigma values differ" % ((got != want).sum(), want.size)
    assert d.zero_knowledge == int(zk) and (not zk or d.num_gate_rows < hc.n)
    if not zk:                                                          # the decoding finds the host's partition again, whatever its ids
        decoded = sm.classes_from_sigma(want, k_is_of(d), d.degree_bits)
        assert sorted(sm.wire_partition(decoded, d.degree_bits).values()) == sorted(sm.wire_partition(classes, d.degree_bits).values())
    else:               # the blinding rows and the padding are singletons (generate_copy adds no copy constraint, circuit_builder.rs:418-420)
        _, inverse, counts = np.unique(classes, return_inverse=True, return_counts=True)
        size = counts[inverse.reshape(classes.shape)]
        assert (size[:, d.num_gate_rows:] == 1).all() and (size[:, :d.num_gate_rows] > 1).any()


# ------------------------------------------------------------------------------- the model against the ext-gate builder
def union_find_sets(c):
    """the builder's own sets of two and more wires (row, column), from its parent table"""
    sets = {}
    for w in list(c.parent):
        sets.setdefault(c._find(w), set()).add(w)
    return sorted(sorted(s) for s in sets.values() if len(s) > 1)


@pytest.mark.parametrize("name,build", [
    ("chained, n = 16", lambda: egc.Chained(seed=1).circuit),
    ("chained, n = 32", lambda: egc.Chained(seed=2, min_degree_bits=5).circuit),
    ("isolated", lambda: egc.isolated([egc.ARITHMETIC_EXT, egc.MUL_EXT, egc.REDUCING, egc.REDUCING_EXT], seed=3)),
])
def test_model_sigma_of_the_ext_gate_circuits_is_a_permutation_whose_cycles_are_the_classes(name, build):
    c = build()
    d = c.desc
    sigma = sm.sigma_values(c.classes, k_is_of(d), d.degree_bits)
    cycles = sm.cycles_of_sigma(sigma, k_is_of(d), d.degree_bits)       # raises unless sigma is a bijection on {k_c w^r}
    assert sum(len(cy) for cy in cycles) == 80 * c.n
    assert sorted(sorted(cy) for cy in cycles if len(cy) > 1) == union_find_sets(c)
    assert all(cy == sorted(cy) for cy in cycles)                       # each cycle walks its wires in (row, column) order
    if name.startswith("chained"):
        assert max(len(cy) for cy in cycles) > 20                       # x is routed into every m1
    else:
        assert [len(cy) for cy in cycles if len(cy) > 1] == [5]         # only the public-input row's zeros are tied


# ------------------------------------------------------------------------------- the guard on the crafted partitions
def class_table(classes):
    """id -> the q = row * 80 + column of its members, ascending"""
    ids = np.ascontiguousarray(np.asarray(classes, dtype=U64).T).reshape(-1).tolist()
    table = {}
    for q, ident in enumerate(ids):
        table.setdefault(ident, []).append(q)
    return ids, table


@pytest.mark.parametrize("lg_n", sc.SIZES)
def test_the_crafted_partitions_have_the_properties_the_gpu_cases_rely_on(lg_n):
    n = 1 << lg_n
    total = 80 * n
    for name in sc.NAMES:
        c = sc.partition(name, lg_n)
        assert c.shape == (80, n) and c.dtype == U64 and (c == sc.partition(name, lg_n)).all(), name      # seeded

    ids, table = class_table(sc.partition("singletons, ids descending", lg_n))
    assert ids == [2**64 - 1 - q for q in range(total)]
    order, _ = sc.sorted_ids(sc.partition("singletons, ids descending", lg_n))
    assert order.tolist() == list(range(total))[::-1]                   # the sort reverses the whole array

    ids, table = class_table(sc.partition("one class", lg_n))
    assert len(table) == 1

    ids, table = class_table(sc.partition("one class per row", lg_n))
    assert sorted(table.values()) == [list(range(80 * r, 80 * r + 80)) for r in range(n)]                # contiguous in the sort's input
    by_row = [ids[80 * r] for r in range(n)]
    assert by_row != sorted(by_row)                                     # and the sort has rows to move

    ids, table = class_table(sc.partition("one class per column, ids col << 32", lg_n))
    assert sorted(table.values()) == [list(range(col, total, 80)) for col in range(80)]                  # members 80 apart
    assert all(ident & 0xFFFFFFFF == 0 for ident in table) and len({ident >> 32 for ident in table}) == 80
    ids, table = class_table(sc.partition("one class per column, ids col", lg_n))
    assert sorted(table.values()) == [list(range(col, total, 80)) for col in range(80)]
    assert all(ident >> 32 == 0 for ident in table) and len(table) == 80

    # ---- the one-bit pairs: none at degree_bits 1 (160 wires cannot hold 128 classes of two), 64 pairs at every other size
    classes, pairs = sc.one_bit_pairs(lg_n)
    ids, table = class_table(classes)
    k = sc.pair_members(lg_n)
    assert (k == 0) == (lg_n == 1) and len(pairs) == (64 if k else 0)
    if k:
        assert len({ident for pair in pairs for ident in pair}) == 128
        for b, (lo, hi) in enumerate(pairs):
            assert lo ^ hi == 1 << b
            for ident in (lo, hi):
                assert len(table[ident]) == k >= 2 and len({q // 80 for q in table[ident]}) == k         # one member per row, k rows
            both = sorted(table[lo] + table[hi])                    # the two interleave in the sort's input: a sort blind to bit b merges them
            assert table[lo] == both[0::2] and table[hi] == both[1::2]
        assert len(table) == 128 + total - 128 * k and total - 128 * k >= 64                              # singletons beside them
    else:
        assert len(table) == total

    # ---- the random partition
    ids, table = class_table(sc.partition("random", lg_n))
    sizes = sorted(len(v) for v in table.values())
    want = sc.random_class_sizes(total)
    singletons = sizes.count(1)
    assert sizes == [1] * singletons + sorted(want) and 0.69 * total <= singletons <= 0.71 * total
    present = {2: True, 3: True, 8: lg_n >= 2, 80: lg_n >= 5, 257: lg_n >= 11}                            # what each size has room for
    for s in sc.CLASS_SIZES:
        assert (s in want[1:]) == present[s], (lg_n, s)
    assert want[0] == total // 4 and sizes[-1] == total // 4
    assert len(table[0]) == 3 and any(q != 0 for q in table[0]) and len(table[2**64 - 1]) == 2
    order, sorted_id = sc.sorted_ids(sc.partition("random", lg_n))
    assert sorted_id[0] == sorted_id[1] == 0 and sorted_id[-1] == sorted_id[-2] == U64(2**64 - 1)       # runs at position 0 and at the last
    quarter = next(v for v in table.values() if len(v) == total // 4)
    assert len({q // 80 for q in quarter}) > n // 2 and len({q % 80 for q in quarter}) > 20               # members at random positions
    if lg_n == 1:
        assert total < 256                                              # no sorted position 256 to cross
    else:
        run = [int(q) for q in order[sc.STRADDLE_START:sc.STRADDLE_START + total // 4]]
        assert sc.STRADDLE_START < 255 and sc.STRADDLE_START + total // 4 > 257 and run == quarter       # one class across positions 255 / 256
        assert sorted_id[sc.STRADDLE_START - 1] != sorted_id[sc.STRADDLE_START] != sorted_id[sc.STRADDLE_START + total // 4]


def test_the_high_word_relabelling_is_a_bijection_that_empties_the_low_word():
    ids = np.array([0, 1, 79, 2**32 - 1, 2**32, 2**64 - 1], dtype=U64)
    assert sc.high_word_relabel(ids).tolist() == [0, 2**32, 79 << 32, (2**32 - 1) << 32, 1, 2**64 - 1]
    assert (sc.high_word_relabel(sc.high_word_relabel(ids)) == ids).all()
