"""The crafted inputs of the lookup tests (no tests here).  A case is a function of n -> (inputs, table), two lists of n 64-bit words;
CASES maps its name to it.  is_valid(inputs, table) is the lookup's own meaning of valid: every input value stands in the table.
INVALID names the cases that are invalid at every n; every other case is valid wherever is_valid says so (a few degenerate at n <= 2).

The device scans run over the 2 n places of the merge of the two sorted columns in segments of SEG places, and a workgroup covers 256
threads: the run and cross-segment cases put their runs and their push / pop pairs across those boundaries where n is large enough.
"""
import numpy as np

P = 0xFFFFFFFF00000001
SEG = 2048                      # GLK_SEG of csrc/stark_lookup_kernels.cuh
B = 1 << 40                     # "large"


def is_valid(inputs, table):
    return {int(x) % P for x in inputs} <= {int(x) % P for x in table}


def _rng(n, salt):
    return np.random.Generator(np.random.PCG64(977 * n + salt))


def _draw(rng, pool, n):
    return [int(pool[int(k)]) for k in rng.integers(0, len(pool), size=n)]


def _range_check(r_of_n, salt):
    def case(n):
        r = max(1, min(n, r_of_n(n)))
        return [int(v) for v in _rng(n, salt).integers(0, r, size=n)], [min(i, r - 1) for i in range(n)]
    return case


def _all_equal(pick):
    def case(n):
        table = [5 + 3 * i for i in range(n)]
        return [table[pick(n)]] * n, table
    return case


def deep_stack(n):
    """table 0 .. n-2, B; inputs all n/2: one Equal, n/2 LIFO pops in descending order, then the deferred fill in ascending order"""
    return [n // 2] * n, list(range(n - 1)) + [B]


def below(n):
    """every input below the table: every pop is deferred on an empty stack"""
    return [int(v) for v in _rng(n, 1).integers(0, n, size=n)], [n + 10 + i for i in range(n)]


def above(n):
    """every input above the table: the first input pushes the whole table, the loop leaves at j == n, every pop is dead over a full stack"""
    return [n + 5 + int(v) for v in _rng(n, 2).integers(0, n, size=n)], list(range(n))


def table_of_one_value(n):
    return [7] * n, [7] * n


def table_of_one_value_mixed_inputs(n):
    return [6 + i % 3 for i in range(n)], [7] * n


def _one_wrong(wrong_of_table, salt):
    def case(n):
        table = [10 + 2 * i for i in range(n)]
        rng = _rng(n, salt)
        inputs = _draw(rng, table, n)
        inputs[int(rng.integers(0, n))] = wrong_of_table(table)
        return inputs, table
    return case


def non_canonical(n):
    """p, p + 1 and 2^64 - 1 on both sides beside their canonical equals 0, 1 and 2^32 - 2"""
    words = [P, 0, P + 1, 1, 2**64 - 1, 2**32 - 2]
    return [words[(5 * i + 3) % 6] for i in range(n)], [words[i % 6] for i in range(n)]


def non_canonical_inputs_only(n):
    return [[P, P + 1, 2**64 - 1][i % 3] for i in range(n)], [[0, 1, 2**32 - 2][(i + 1) % 3] for i in range(n)]


def high_values(n):
    table = [2**63 + 3 * i for i in range(n - 1)] + [P - 1]
    return _draw(_rng(n, 3), table, n), table


def one_bit_apart(n):
    """0 and 2^b for every b < 64: neighbours in the order differ in one bit of each of the 64 positions"""
    table = [0 if i % 65 == 64 else 1 << (i % 65) for i in range(n)]
    return _draw(_rng(n, 4), table, n), table


def _run(start_of_n, length=13):
    """inputs i with a run of `length` equal values from sorted position `start` on; table 0 .. n-1"""
    def case(n):
        ln = max(1, min(length, n))
        start = max(0, min(start_of_n(n), n - ln))
        return [start if start <= i < start + ln else i for i in range(n)], list(range(n))
    return case


def table_runs(n):
    """runs of equal TABLE values (pushes) at the first and the last sorted positions, inputs from the middle"""
    r = max(1, n // 4)
    table = [0] * r + list(range(1, n - 2 * r + 1)) + [n] * r
    table = (table + [n] * n)[:n]
    return _draw(_rng(n, 5), table[r:n - r] or table, n), table


def sawtooth(n):
    """table i, inputs 1 1 3 3 5 5 ..: push, Equal, pop, over and over on ONE level: its events lie in every scan segment"""
    return [(i // 2) * 2 + 1 if (i // 2) * 2 + 1 < n else n - 1 for i in range(n)], list(range(n))


def sawtooth_invalid(n):
    """table 4 i, inputs 4 i + 2: push, pop, push, pop .. on one level, no input in the table"""
    return [4 * i + 2 for i in range(n)], [4 * i for i in range(n)]


def nested(n):
    """table i; inputs: n/4 copies each of n/4 and 3n/4 and n/2 other values: two stacks of pushes popped far from where they were pushed"""
    q = max(1, n // 4)
    inputs = [q] * q + [min(n - 1, 3 * q)] * q
    inputs += _draw(_rng(n, 6), list(range(n)), n)
    return inputs[:n], list(range(n))


def random_valid(n):
    rng = _rng(n, 7)
    table = [int(v) for v in rng.integers(0, max(2, n // 2), size=n)]
    return _draw(rng, table, n), table


def random_any(n):
    rng = _rng(n, 8)
    return [int(v) for v in rng.integers(0, n + 2, size=n)], [int(v) for v in rng.integers(0, n + 2, size=n)]


def random_full_width(n):
    rng = _rng(n, 9)
    table = [int(v) for v in rng.integers(0, 2**64, size=n, dtype=np.uint64)]
    return [int(v) + (P if int(v) < 2**32 - 1 and k % 2 else 0) for k, v in enumerate(_draw(rng, [t % P for t in table], n))], table


CASES = {
    "range-check-R1": _range_check(lambda n: 1, 11),
    "range-check-R2": _range_check(lambda n: 2, 12),
    "range-check-Rhalf": _range_check(lambda n: n // 2, 13),
    "range-check-Rn": _range_check(lambda n: n, 14),
    "all-equal-smallest": _all_equal(lambda n: 0),
    "all-equal-middle": _all_equal(lambda n: n // 2),
    "all-equal-largest": _all_equal(lambda n: n - 1),
    "deep-stack": deep_stack,                                   # its first push and its last pop are n places apart: two scan segments from n = SEG on
    "below": below,
    "above": above,
    "table-of-one-value": table_of_one_value,
    "table-of-one-value-mixed-inputs": table_of_one_value_mixed_inputs,
    "invalid-above-the-maximum": _one_wrong(lambda t: t[-1] + 1, 15),
    "invalid-below-the-minimum": _one_wrong(lambda t: t[0] - 1, 16),
    "invalid-in-a-gap": _one_wrong(lambda t: t[len(t) // 2] + 1, 17),
    "non-canonical": non_canonical,
    "non-canonical-inputs-only": non_canonical_inputs_only,
    "high-values": high_values,
    "one-bit-apart": one_bit_apart,
    "run-first": _run(lambda n: 0, 40),
    "run-last": _run(lambda n: n, 40),
    "run-across-256": _run(lambda n: 250),                      # sorted positions 250 .. 262
    "run-across-256-places": _run(lambda n: 122),               # merge places 244 .. 269: the workgroup boundary of the classify launch
    "run-across-a-scan-segment": _run(lambda n: SEG // 2 - 6),  # merge places about SEG - 12 .. SEG + 14
    "run-across-the-second-scan-segment": _run(lambda n: SEG - 6),
    "table-runs": table_runs,
    "sawtooth-one-level-in-every-segment": sawtooth,
    "sawtooth-invalid": sawtooth_invalid,
    "nested": nested,
    "random-valid": random_valid,
    "random-any": random_any,
    "random-full-width": random_full_width,
}
INVALID = ("below", "above", "table-of-one-value-mixed-inputs", "invalid-above-the-maximum", "invalid-below-the-minimum", "invalid-in-a-gap", "sawtooth-invalid")


def case(name, n):
    inputs, table = CASES[name](n)
    assert len(inputs) == len(table) == n and all(0 <= int(x) < 2**64 for x in inputs + table), name
    return inputs, table


# ------------------------------------------------------------------------------- the range-check AIR of the end-to-end tests
VALUE, COUNTER, PERMUTED_VALUE, PERMUTED_COUNTER = range(4)


def range_check_air(lookup_constraints, r):
    """value in [0, r) by a lookup into a counter column, as ArithmeticStark does it (arithmetic_stark.rs:97-118, 147-170): the counter
    starts at 0, steps by 0 or 1 and ends at r - 1; eval_lookups on the permuted columns; the two permutations as
    MemoryStark::permutation_pairs states them (memory_stark.rs:283-294).  In the shape of stark_airs.py."""
    from stark_airs import FIRST_ROW, LAST_ROW, M1, TRANSITION, L, N, _air
    c = COUNTER
    constraints = [
        (FIRST_ROW, [(1, [L(c)])]),
        (TRANSITION, [(1, [N(c), N(c)]), (P - 2, [N(c), L(c)]), (1, [L(c), L(c)]), (M1, [N(c)]), (1, [L(c)])]),      # d (d - 1), d = next - local
        (LAST_ROW, [(1, [L(c)]), ((P - (r - 1)) % P, [])]),
    ] + lookup_constraints(PERMUTED_VALUE, PERMUTED_COUNTER)
    return _air("range-check", 4, 0, 3, 1, constraints, [[(VALUE, PERMUTED_VALUE)], [(COUNTER, PERMUTED_COUNTER)]], None)


def range_check_columns(n, r, seed=0):
    """-> (value column, counter column)"""
    return [int(v) for v in _rng(n, 100 + seed).integers(0, r, size=n)], [min(i, r - 1) for i in range(n)]
