"""Crafted memory-operation logs for the memory table's tests (no tests here).  A log is a list of memory_model.op dicts in ISSUE order;
records(log) packs it as the library takes it.  Every log of CASES is a consistent memory log (a read returns what the last write to
its address stored), so its trace satisfies MemoryStark's constraints; REFUSED holds logs the reference's assertion turns away, and
mismatched_read() one that generates but cannot be proved.  Heights stay at or below 2^13 rows."""
import numpy as np

import memory_model as mm
from memory_model import op

SEG = 2048                                                              # places per segment of the kernels' scan
B31 = 1 << 31


def records(log):
    import plonky2_demo_amd as p
    a = np.zeros(len(log), dtype=p.MEMORY_OP_DTYPE)
    for k, o in enumerate(log):
        a[k] = (o["filter"], o["is_read"], o["context"], o["segment"], o["virt"], o["timestamp"], o["value"])
    return a


def W(context, segment, virt, timestamp, value):
    return op(context, segment, virt, timestamp, value, is_read=0)


def R(context, segment, virt, timestamp, value):
    return op(context, segment, virt, timestamp, value, is_read=1)


BIG = (1 << 256) - 0x1234567                                            # a value with every limb in use


def random_log(num_ops, seed, virts=None, shuffle=True):
    """a consistent log: accesses to a small set of addresses with a clock that only goes forward (so an address never sees one
    timestamp twice and the issue order may be shuffled)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    virts = list(virts) if virts is not None else list(range(12)) + [40, 41, 300]
    memory, log, clock = {}, [], 0
    for _ in range(num_ops):
        clock += int(rng.integers(1, 4))
        address = (int(rng.integers(0, 3)), int(rng.integers(0, 3)), virts[int(rng.integers(0, len(virts)))])
        if address not in memory or rng.integers(0, 3) == 0:
            value = int.from_bytes(rng.bytes(32), "little")
            if address in memory or rng.integers(0, 2):
                memory[address] = value
                log.append(W(*address, clock, value))
                continue
            memory[address] = value                                     # a first read: whatever it returns is what later reads see
        log.append(R(*address, clock, memory[address]))
    if shuffle:
        log = [log[int(k)] for k in rng.permutation(len(log))]
    return log


def _cases():
    c = {}
    c["one-op"] = [W(3, 1, 7, 12, BIG)]
    c["two-ops"] = [R(0, 0, 5, 9, 77), W(0, 0, 5, 8, 77)]
    c["three-ops"] = [W(1, 2, 3, 1, 5), R(1, 2, 3, 2, 5), W(1, 2, 4, 3, BIG)]
    c["first-change-in-each-part"] = [W(0, 0, 0, 1, 1), W(0, 0, 1, 2, 2), W(0, 1, 0, 3, 3), W(1, 0, 0, 4, 4), R(1, 0, 0, 5, 4), W(1, 2, 0, 6, 5), W(3, 0, 0, 7, 6)]
    # parts that differ only in bit 31, each behind a change of an earlier part (a step of 2^31 in context or segment is refused, in virt
    # or timestamp it asks for 2^31 / max_rc rows): the sort keys must carry all 32 bits of every part
    c["bit-31"] = [W(B31 + 1, B31 + 8, B31 + 9, 6, 4), W(B31 + 1, B31 + 7, 10, 5, 3), W(B31, 7, B31 + 9, 5, 1), W(B31 + 1, B31 + 7, 9, B31 + 5, 2)]
    c["ties-with-different-values-and-kinds"] = [W(0, 0, 1, 4, 10), W(0, 0, 1, 4, 11), R(0, 0, 1, 4, 11), W(0, 0, 1, 4, BIG), R(0, 0, 1, 4, BIG), W(0, 0, 0, 4, 9)]
    # four ops: max_rc = 3
    c["virt-gap-of-max-rc"] = [W(0, 0, 0, 1, 1), W(0, 0, 4, 2, 2), W(0, 0, 5, 3, 3), W(0, 0, 6, 4, 4)]
    c["virt-gap-of-max-rc-plus-one"] = [W(0, 0, 0, 1, 1), W(0, 0, 5, 2, 2), W(0, 0, 6, 3, 3), W(0, 0, 7, 4, 4)]
    c["timestamp-gap-of-max-rc"] = [W(0, 0, 0, 1, 8), R(0, 0, 0, 4, 8), R(0, 0, 0, 5, 8), R(0, 0, 0, 6, 8)]
    c["timestamp-gap-of-max-rc-plus-one"] = [W(0, 0, 0, 1, 8), R(0, 0, 0, 5, 8), R(0, 0, 0, 6, 8), R(0, 0, 0, 7, 8)]
    # the doc comment's example (memory_stark.rs:160-162): 32 ops, one address accessed at timestamps 20 and 100
    c["timestamps-20-and-100"] = [W(0, 0, 1, 20, BIG), R(0, 0, 1, 100, BIG)] + [W(0, 0, 2 + k, 30 + k, k) for k in range(30)]
    c["gap-rows-push-the-height-over-a-power-of-two"] = [W(0, 0, 0, 1, 1), W(0, 0, 1, 2, 2), W(0, 0, 2, 3, 3), R(0, 0, 2, 40, 3)]
    # two ops, max_rc = 1: 5000 rows between them, the height 2^13
    c["one-pair-asks-for-5000-rows"] = [W(2, 1, 6, 3, BIG), R(2, 1, 6, 5004, BIG)]
    c["one-virt-pair-asks-for-5000-rows"] = [W(2, 1, 6, 3, BIG), W(2, 1, 6 + 2 * 5000 + 1, 4, 7)]
    c["dummies-from-several-pairs-padding-mid-trace"] = [W(0, 0, 0, 1, 1), R(0, 0, 0, 30, 1), W(0, 0, 50, 2, 2), W(0, 1, 0, 3, 3), R(0, 1, 0, 20, 3), W(1, 0, 0, 5, 4),
                                                         W(1, 0, 1, 6, 5)]
    c["no-dummies-padding-behind-a-tie"] = [W(0, 0, 0, 1, 1), W(0, 0, 1, 2, 2), W(0, 0, 1, 2, 3)]
    c["read-after-write"] = [W(0, 0, 3, 1, BIG), R(0, 0, 3, 2, BIG), R(0, 0, 3, 3, BIG), W(0, 0, 3, 4, 6), R(0, 0, 3, 5, 6)]
    c["writes-only"] = [W(0, 0, k % 3, k, k * k + 1) for k in range(1, 7)]
    for num_ops in (255, 256, 257):
        c["random-%d" % num_ops] = random_log(num_ops, seed=num_ops, virts=list(range(10)) + [600, 601, 1500])
    for num_ops in (SEG - 1, SEG, SEG + 1):
        c["random-%d" % num_ops] = random_log(num_ops, seed=num_ops, virts=list(range(40)) + [5000, 5001, 30000])
    return c


CASES = _cases()


def mismatched_read():
    """a read that returns what its preceding write did not store: generate_trace does not complain, the constraints do"""
    return [W(0, 0, k, 1 + k, 100 + k) for k in range(20)] + [R(0, 0, 7, 40, 100 + 7 + 1)]


# logs on which the assertion of memory_stark.rs:112-116 fails: a context or segment step, minus one, that is >= the height
REFUSED = {
    "context-step": [W(0, 0, 0, 1, 1), W(5, 0, 0, 2, 2), W(5, 0, 1, 3, 3), W(5, 0, 2, 4, 4)],          # 5 - 0 - 1 = 4 >= 4
    "segment-step": [W(0, 0, 0, 1, 1), W(0, 9, 0, 2, 2)],
    "context-bit-31": [W(1, 0, 0, 1, 1), W(B31 + 1, 0, 0, 2, 2), W(2, 0, 0, 3, 3)],
}
# ... and the largest steps it lets through
ALLOWED_STEPS = {
    "context-step": [W(0, 0, 0, 1, 1), W(4, 0, 0, 2, 2), W(4, 0, 1, 3, 3), W(4, 0, 2, 4, 4)],          # 4 - 0 - 1 = 3 < 4
    "segment-step": [W(0, 0, 0, 1, 1), W(0, 2, 0, 2, 2)],
}
# a log that asks for 2^31 rows (one pair, two ops: max_rc = 1) and one just above 2^24
TOO_HIGH = {
    "2^31-rows": [W(0, 0, 0, 0, 1), R(0, 0, 0, B31 + 1, 1)],
    "2^24-plus-one": [W(0, 0, 0, 0, 1), W(0, 0, 2 * ((1 << 24) - 1) + 1, 1, 1)],
}


def dag_desc(p):
    """MemoryStark stated a second time, the way eval_packed_generic is written (memory_stark.rs:243-321) with its shared subexpressions,
    through StarkDagBuilder: the same polynomials as the term lists gl_memory_stark_desc exports, so the same proof bytes"""
    b = p.StarkDagBuilder(mm.NUM_COLUMNS, 0)
    one = b.const(1)
    timestamp, addr_context, addr_segment, addr_virtual = b.local(mm.TIMESTAMP), b.local(mm.ADDR_CONTEXT), b.local(mm.ADDR_SEGMENT), b.local(mm.ADDR_VIRTUAL)
    values = [b.local(mm.value_limb(i)) for i in range(8)]
    next_timestamp, next_is_read = b.next(mm.TIMESTAMP), b.next(mm.IS_READ)
    next_addr_context, next_addr_segment, next_addr_virtual = b.next(mm.ADDR_CONTEXT), b.next(mm.ADDR_SEGMENT), b.next(mm.ADDR_VIRTUAL)
    next_values = [b.next(mm.value_limb(i)) for i in range(8)]
    filt = b.local(mm.FILTER)
    b.constraint(filt * (filt - one))
    is_dummy, is_write = one - filt, one - b.local(mm.IS_READ)
    b.constraint(is_dummy * is_write)
    context_first_change, segment_first_change, virtual_first_change = b.local(mm.CONTEXT_FIRST_CHANGE), b.local(mm.SEGMENT_FIRST_CHANGE), b.local(mm.VIRTUAL_FIRST_CHANGE)
    address_unchanged = one - context_first_change - segment_first_change - virtual_first_change
    range_check = b.local(mm.RANGE_CHECK)
    b.constraint(context_first_change * (one - context_first_change))
    b.constraint(segment_first_change * (one - segment_first_change))
    b.constraint(virtual_first_change * (one - virtual_first_change))
    b.constraint(address_unchanged * (one - address_unchanged))
    b.constraint_transition(segment_first_change * (next_addr_context - addr_context))
    b.constraint_transition(virtual_first_change * (next_addr_context - addr_context))
    b.constraint_transition(virtual_first_change * (next_addr_segment - addr_segment))
    b.constraint_transition(address_unchanged * (next_addr_context - addr_context))
    b.constraint_transition(address_unchanged * (next_addr_segment - addr_segment))
    b.constraint_transition(address_unchanged * (next_addr_virtual - addr_virtual))
    computed_range_check = (context_first_change * (next_addr_context - addr_context - one) + segment_first_change * (next_addr_segment - addr_segment - one)
                            + virtual_first_change * (next_addr_virtual - addr_virtual - one) + address_unchanged * (next_timestamp - timestamp))
    b.constraint_transition(range_check - computed_range_check)
    for i in range(8):
        b.constraint_transition(next_is_read * address_unchanged * (next_values[i] - values[i]))
    diff_input_prev = b.next(mm.RANGE_CHECK_PERMUTED) - b.local(mm.RANGE_CHECK_PERMUTED)      # eval_lookups, lookup.rs:13-34
    diff_input_table = b.next(mm.RANGE_CHECK_PERMUTED) - b.next(mm.COUNTER_PERMUTED)
    b.constraint(diff_input_prev * diff_input_table)
    b.constraint_last_row(diff_input_table)
    return b.build(3, [[(mm.RANGE_CHECK, mm.RANGE_CHECK_PERMUTED)], [(mm.COUNTER, mm.COUNTER_PERMUTED)]])


def end_to_end_log(lg_n):
    """a consistent log whose trace has 2^lg_n rows, some of them pushed by fill_gaps"""
    if lg_n == 12:
        return CASES["random-%d" % (SEG + 1)]
    # 22 ops, max_rc = 31: a virt step to 100 and a timestamp step of 70 at one address push rows; 32 rows in all
    return random_log(20, seed=3, virts=range(6)) + [W(0, 0, 100, 200, BIG), R(0, 0, 100, 270, BIG)]
