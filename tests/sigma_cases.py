"""Crafted copy-constraint partitions for the sigma kernels (csrc/sigma.hip), by name and size (no tests here).

Every partition is a seeded construction: classes [80][n] of u64 ids, nothing repaired afterwards.  tests/test_sigma_model.py holds the guard
that asserts, on the CPU and for every size, the properties tests/test_sigma.py relies on; the names in WHY say what each one is for.
"Sorted position": the place of a wire after the kernels' stable sort by id of the wires enumerated in (row, column) order.
"""
import numpy as np

NUM_ROUTED = 80
U64 = np.uint64
MAX_ID = 2**64 - 1
SIZES = [1, 2, 5, 11, 12]               # degree_bits: 160 wires (under one 256-thread block), 320 (a block boundary inside), 2560, n = 2048
                                        # (row >> 11 is 0 everywhere), n = 4096 (a second xpow_hi entry; 327,680 wires: hipcub's multi-block sort)
WHY = {
    "singletons, ids descending": "ids 2^64 - 1 - q in enumeration order: the sort reverses the whole array, sigma is the identity",
    "one class": "all 80 n wires in one run: no head but position 0, the wrap from the last position to the first",
    "one class per row": "members contiguous in the sort's input",
    "one class per column, ids col << 32": "members 80 apart in the sort's input (stability); the ids differ only in the high word",
    "one class per column, ids col": "members 80 apart in the sort's input (stability); the ids differ only in the low word",
    "one-bit id pairs": "64 pairs of classes whose ids differ in exactly bit b, b = 0..63, singletons beside them",
    "random": "70 % singletons, classes of 2, 3, 8, 80, 257 and a quarter of all wires at random positions, ids 0 and 2^64 - 1 present",
}
NAMES = list(WHY)
PAIR_BITS = 64
CLASS_SIZES = [2, 3, 8, 80, 257]
STRADDLE_START = 236                    # the sorted position at which the quarter class of the random partition starts (sizes with > 256 wires)


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def random_ids(rng, k):
    return [int(v) for v in rng.integers(0, MAX_ID, size=k, dtype=U64, endpoint=True)]


def wire_of(q):
    """the q-th wire in (row, column) order"""
    return divmod(q, NUM_ROUTED)


def _matrix(ids_by_q, n):
    """ids indexed by q = row * 80 + column -> classes [80][n]"""
    return np.array(ids_by_q, dtype=U64).reshape(n, NUM_ROUTED).T.copy()


def pair_members(lg_n):
    """members per class of the one-bit pairs: 0 where 128 classes of two do not fit, else 2 to 5"""
    total = NUM_ROUTED << lg_n
    return 0 if total < 2 * 2 * PAIR_BITS else min(5, total // (2 * 2 * PAIR_BITS) + 1)


def one_bit_pairs(lg_n, seed=7300):
    """-> (classes, [(id, id ^ 1 << b)] for b = 0..63).  Pair b owns the 2 k slots s = 2 k b + t, slot s being the wire in row rows[s % n],
    column cols[s // n] for a seeded shuffle of the rows and of the columns: 2 k <= n wires in 2 k different rows.  In (row, column) order they
    go to the two classes in turn, so that each class has k members in k rows and the two interleave in the sort's input: a sort that
    does not see bit b merges them into one run.  Every other wire is a singleton with a seeded 64-bit id."""
    n, rng = 1 << lg_n, rng_of(seed + lg_n)
    total, k = NUM_ROUTED * n, pair_members(lg_n)
    ids = random_ids(rng, total)
    pairs = []
    if k:
        assert 2 * k <= n and 2 * PAIR_BITS * k <= total
        rows, cols = rng.permutation(n), rng.permutation(NUM_ROUTED)
        bases = random_ids(rng, PAIR_BITS)
        pairs = [(bases[b], bases[b] ^ (1 << b)) for b in range(PAIR_BITS)]
        for b in range(PAIR_BITS):
            slots = range(2 * k * b, 2 * k * (b + 1))
            for t, q in enumerate(sorted(int(rows[s % n]) * NUM_ROUTED + int(cols[s // n]) for s in slots)):
                ids[q] = pairs[b][t % 2]
    return _matrix(ids, n), pairs


def random_class_sizes(total):
    """the sizes of the random partition's classes of two and more: a quarter of all wires, then 2, 3, 8, 80, 257 in turn (a size that no
    longer fits is passed over) until 30 % of the wires are used"""
    sizes, left = [total // 4], total * 3 // 10 - total // 4
    while left >= 2:
        for s in CLASS_SIZES:
            if s <= left:
                sizes.append(s)
                left -= s
    return sizes


def random_partition(lg_n, seed=7400):
    """Members at seeded random positions (slices of one shuffle of all wires), seeded 64-bit ids.  The first class of 3 has id 0 and the
    first class of 2 has id 2^64 - 1: a run of several wires starts at sorted position 0 and another ends at the last one.  Where there are
    more than 256 wires, the id of the quarter class is placed by construction: one above the id that holds sorted position
    STRADDLE_START - 1 among all other wires, so that its run starts at STRADDLE_START and crosses sorted positions 255 / 256."""
    n, rng = 1 << lg_n, rng_of(seed + lg_n)
    total = NUM_ROUTED * n
    sizes, order = random_class_sizes(total), rng.permutation(total)
    ids = random_ids(rng, total)                                    # singletons unless overwritten below
    class_ids = random_ids(rng, len(sizes))
    class_ids[sizes.index(3)], class_ids[sizes.index(2)] = 0, MAX_ID
    at = sizes[0]
    for s, ident in zip(sizes[1:], class_ids[1:]):
        for q in order[at:at + s]:
            ids[int(q)] = ident
        at += s
    quarter = [int(q) for q in order[:sizes[0]]]
    if total > 256:
        others = sorted(set(range(total)) - set(quarter), key=lambda q: ids[q])
        class_ids[0] = ids[others[STRADDLE_START - 1]] + 1
    for q in quarter:
        ids[q] = class_ids[0]
    return _matrix(ids, n)


def partition(name, lg_n):
    """classes [80][n] u64 of the partition `name` at n = 2^lg_n"""
    n = 1 << lg_n
    total = NUM_ROUTED * n
    if name == "singletons, ids descending":
        return _matrix([MAX_ID - q for q in range(total)], n)
    if name == "one class":
        return _matrix(random_ids(rng_of(7100 + lg_n), 1) * total, n)
    if name == "one class per row":                                 # an odd multiplier: a bijection of the rows; the last row has id 0
        return _matrix([(n - 1 - wire_of(q)[0]) * 0x9E3779B97F4A7C15 % 2**64 for q in range(total)], n)
    if name == "one class per column, ids col << 32":
        return _matrix([wire_of(q)[1] << 32 for q in range(total)], n)
    if name == "one class per column, ids col":
        return _matrix([wire_of(q)[1] for q in range(total)], n)
    if name == "one-bit id pairs":
        return one_bit_pairs(lg_n)[0]
    if name == "random":
        return random_partition(lg_n)
    raise KeyError(name)


def sorted_ids(classes):
    """-> (the wires' q = row * 80 + column in the order of the stable sort by id, their ids in that order)"""
    ids = np.ascontiguousarray(np.asarray(classes, dtype=U64).T).reshape(-1)
    order = np.argsort(ids, kind="stable")
    return order, ids[order]


def high_word_relabel(classes):
    """ids rotated by 32 bits: a bijection of the u64 that moves what differs in the low word into the high word"""
    c = np.asarray(classes, dtype=U64)
    return (c << U64(32)) | (c >> U64(32))
