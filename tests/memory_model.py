"""A plain Python-integer model of evm's memory table (no tests here), transcribed from the reference statement by statement:
  witness/memory.rs:80-125                 MemoryOp, new_dummy_read, sorting_key
  memory/memory_stark.rs:52-70             into_row
  memory/memory_stark.rs:73-118            generate_first_change_flags_and_rc, with its assertion
  memory/memory_stark.rs:123-237           generate_trace: the stable sort, fill_gaps, pad_memory_ops, the second sort, COUNTER, permuted_cols
  memory/memory_stark.rs:243-321           eval_packed_generic, written the way the Rust is over the Base / Ext fields of stark_model
The SEQUENTIAL loops, not the kernels' formulation (prefix sums over per-pair counts): the kernels are judged against the reference's
own semantics.  An op is a dict with the fields of gl_memory_op (value: eight 32-bit limbs); field elements are Python integers.
"""
import lookup_model as lm
from lookup_model import P

NUM_CHANNELS = 6
(FILTER, TIMESTAMP, IS_READ, ADDR_CONTEXT, ADDR_SEGMENT, ADDR_VIRTUAL) = range(6)
VALUE_LIMBS = 8


def value_limb(i):
    return 6 + i


CONTEXT_FIRST_CHANGE = 6 + VALUE_LIMBS
SEGMENT_FIRST_CHANGE = CONTEXT_FIRST_CHANGE + 1
VIRTUAL_FIRST_CHANGE = SEGMENT_FIRST_CHANGE + 1
RANGE_CHECK = VIRTUAL_FIRST_CHANGE + NUM_CHANNELS
COUNTER = RANGE_CHECK + 1
RANGE_CHECK_PERMUTED = COUNTER + 1
COUNTER_PERMUTED = RANGE_CHECK_PERMUTED + 1
NUM_COLUMNS = COUNTER_PERMUTED + 1


class RangeCheckTooLarge(AssertionError):
    """memory_stark.rs:112-116"""


def op(context, segment, virt, timestamp, value=0, is_read=1, filter=1):
    """a MemoryOp; value: an integer below 2^256 or eight limbs"""
    limbs = [(value >> (32 * j)) & 0xFFFFFFFF for j in range(8)] if isinstance(value, int) else [int(v) for v in value]
    return dict(filter=int(filter), is_read=int(is_read), context=int(context), segment=int(segment), virt=int(virt), timestamp=int(timestamp),
                value=limbs)


def sorting_key(o):
    return (o["context"], o["segment"], o["virt"], o["timestamp"])


def new_dummy_read(address, timestamp, value):
    return dict(filter=0, is_read=1, context=address[0], segment=address[1], virt=address[2], timestamp=timestamp, value=list(value))


def next_power_of_two(k):
    return 1 if k <= 1 else 1 << (k - 1).bit_length()


def fill_gaps(memory_ops):
    """:163-192, pushing onto memory_ops"""
    max_rc = next_power_of_two(len(memory_ops)) - 1
    snapshot = list(memory_ops)                                          # memory_ops.clone().into_iter().tuple_windows()
    for curr, nxt in zip(snapshot, snapshot[1:]):
        if curr["context"] != nxt["context"] or curr["segment"] != nxt["segment"]:
            pass
        elif curr["virt"] != nxt["virt"]:
            while nxt["virt"] - curr["virt"] - 1 > max_rc:
                dummy = new_dummy_read((curr["context"], curr["segment"], curr["virt"] + max_rc + 1), 0, [0] * 8)
                memory_ops.append(dummy)
                curr = dummy
        else:
            while nxt["timestamp"] - curr["timestamp"] > max_rc:
                dummy = new_dummy_read((curr["context"], curr["segment"], curr["virt"]), curr["timestamp"] + max_rc, curr["value"])
                memory_ops.append(dummy)
                curr = dummy


def pad_memory_ops(memory_ops):
    """:194-212"""
    padding = dict(memory_ops[-1], filter=0, is_read=1)
    memory_ops.extend([padding] * (next_power_of_two(len(memory_ops)) - len(memory_ops)))


def into_row(o):
    row = [0] * NUM_COLUMNS
    row[FILTER], row[TIMESTAMP], row[IS_READ] = o["filter"], o["timestamp"], o["is_read"]
    row[ADDR_CONTEXT], row[ADDR_SEGMENT], row[ADDR_VIRTUAL] = o["context"], o["segment"], o["virt"]
    for j in range(VALUE_LIMBS):
        row[value_limb(j)] = o["value"][j]
    return row


def generate_first_change_flags_and_rc(rows):
    """:73-118"""
    num_ops = len(rows)
    for idx in range(num_ops - 1):
        row, nxt = rows[idx], rows[idx + 1]
        context_first_change = row[ADDR_CONTEXT] != nxt[ADDR_CONTEXT]
        segment_first_change = row[ADDR_SEGMENT] != nxt[ADDR_SEGMENT] and not context_first_change
        virtual_first_change = row[ADDR_VIRTUAL] != nxt[ADDR_VIRTUAL] and not segment_first_change and not context_first_change
        row[CONTEXT_FIRST_CHANGE], row[SEGMENT_FIRST_CHANGE], row[VIRTUAL_FIRST_CHANGE] = (int(context_first_change), int(segment_first_change),
                                                                                          int(virtual_first_change))
        if context_first_change:
            rc = nxt[ADDR_CONTEXT] - row[ADDR_CONTEXT] - 1
        elif segment_first_change:
            rc = nxt[ADDR_SEGMENT] - row[ADDR_SEGMENT] - 1
        elif virtual_first_change:
            rc = nxt[ADDR_VIRTUAL] - row[ADDR_VIRTUAL] - 1
        else:
            rc = nxt[TIMESTAMP] - row[TIMESTAMP]
        row[RANGE_CHECK] = rc % P
        if not row[RANGE_CHECK] < num_ops:
            raise RangeCheckTooLarge("Range check of %d is too large. Bug in fill_gaps?" % row[RANGE_CHECK])


def generate_trace(ops):
    """MemoryStark::generate_trace (:214-237) -> [NUM_COLUMNS][n] columns of canonical integers"""
    memory_ops = sorted((dict(o) for o in ops), key=sorting_key)         # sort_by_key is stable, as sorted() is
    fill_gaps(memory_ops)
    pad_memory_ops(memory_ops)
    memory_ops.sort(key=sorting_key)
    rows = [into_row(o) for o in memory_ops]
    generate_first_change_flags_and_rc(rows)
    cols = [list(c) for c in zip(*rows)]
    height = len(cols[0])
    cols[COUNTER] = list(range(height))
    cols[RANGE_CHECK_PERMUTED], cols[COUNTER_PERMUTED] = lm.permuted_cols(cols[RANGE_CHECK], cols[COUNTER])
    return cols


def eval_packed_generic(F, local, nxt):
    """:243-321 over the field F (stark_model.Base / Ext) -> [(filter name, value)] in the order yielded, each BEFORE its filter;
    local / nxt: NUM_COLUMNS elements of F.  eval_lookups (lookup.rs:13-34) comes last."""
    out = []
    one = F.one
    timestamp, addr_context, addr_segment, addr_virtual = local[TIMESTAMP], local[ADDR_CONTEXT], local[ADDR_SEGMENT], local[ADDR_VIRTUAL]
    values = [local[value_limb(i)] for i in range(8)]
    next_timestamp, next_is_read = nxt[TIMESTAMP], nxt[IS_READ]
    next_addr_context, next_addr_segment, next_addr_virtual = nxt[ADDR_CONTEXT], nxt[ADDR_SEGMENT], nxt[ADDR_VIRTUAL]
    next_values = [nxt[value_limb(i)] for i in range(8)]

    def constraint(v):
        out.append(("all", v))

    def constraint_transition(v):
        out.append(("transition", v))
    filt = local[FILTER]
    constraint(F.mul(filt, F.sub(filt, one)))
    is_dummy = F.sub(one, filt)
    is_write = F.sub(one, local[IS_READ])
    constraint(F.mul(is_dummy, is_write))
    context_first_change, segment_first_change, virtual_first_change = local[CONTEXT_FIRST_CHANGE], local[SEGMENT_FIRST_CHANGE], local[VIRTUAL_FIRST_CHANGE]
    address_unchanged = F.sub(F.sub(F.sub(one, context_first_change), segment_first_change), virtual_first_change)
    range_check = local[RANGE_CHECK]
    not_context_first_change = F.sub(one, context_first_change)
    not_segment_first_change = F.sub(one, segment_first_change)
    not_virtual_first_change = F.sub(one, virtual_first_change)
    not_address_unchanged = F.sub(one, address_unchanged)
    constraint(F.mul(context_first_change, not_context_first_change))
    constraint(F.mul(segment_first_change, not_segment_first_change))
    constraint(F.mul(virtual_first_change, not_virtual_first_change))
    constraint(F.mul(address_unchanged, not_address_unchanged))
    constraint_transition(F.mul(segment_first_change, F.sub(next_addr_context, addr_context)))
    constraint_transition(F.mul(virtual_first_change, F.sub(next_addr_context, addr_context)))
    constraint_transition(F.mul(virtual_first_change, F.sub(next_addr_segment, addr_segment)))
    constraint_transition(F.mul(address_unchanged, F.sub(next_addr_context, addr_context)))
    constraint_transition(F.mul(address_unchanged, F.sub(next_addr_segment, addr_segment)))
    constraint_transition(F.mul(address_unchanged, F.sub(next_addr_virtual, addr_virtual)))
    computed_range_check = F.add(F.add(F.add(
        F.mul(context_first_change, F.sub(F.sub(next_addr_context, addr_context), one)),
        F.mul(segment_first_change, F.sub(F.sub(next_addr_segment, addr_segment), one))),
        F.mul(virtual_first_change, F.sub(F.sub(next_addr_virtual, addr_virtual), one))),
        F.mul(address_unchanged, F.sub(next_timestamp, timestamp)))
    constraint_transition(F.sub(range_check, computed_range_check))
    for i in range(8):
        constraint_transition(F.mul(F.mul(next_is_read, address_unchanged), F.sub(next_values[i], values[i])))
    # eval_lookups(vars, yield_constr, RANGE_CHECK_PERMUTED, COUNTER_PERMUTED), lookup.rs:13-34
    diff_input_prev = F.sub(nxt[RANGE_CHECK_PERMUTED], local[RANGE_CHECK_PERMUTED])
    diff_input_table = F.sub(nxt[RANGE_CHECK_PERMUTED], nxt[COUNTER_PERMUTED])
    constraint(F.mul(diff_input_prev, diff_input_table))
    out.append(("last_row", diff_input_table))
    return out
