"""A plain Python-integer model of the Halo2-style lookup of evm/src/lookup.rs (no tests here):
  lookup.rs:65-127   permuted_cols   the SEQUENTIAL loop, transcribed statement by statement: two sorts, the merge with its LIFO stack of
                                     unused table values, the deferred fill.  Not the kernels' parallel formulation: they are judged
                                     against the reference's own semantics.
  lookup.rs:13-34    eval_lookups    the two constraints on a pair of rows.
Field elements are Python integers; inputs may be non-canonical 64-bit words.
"""
P = 0xFFFFFFFF00000001


def permuted_cols(inputs, table):
    """-> (permuted_inputs, permuted_table), canonical integers"""
    n = len(inputs)
    assert len(table) == n
    sorted_inputs = sorted(int(x) % P for x in inputs)                   # :79-83  to_canonical, sorted by to_noncanonical_u64
    sorted_table = sorted(int(x) % P for x in table)                     # :84-88
    unused_table_inds, unused_table_vals = [], []                        # :90-91
    permuted_table = [0] * n                                             # :92
    i = j = 0
    while j < n and i < n:                                               # :95
        input_val, table_val = sorted_inputs[i], sorted_table[j]
        if input_val > table_val:                                        # Ordering::Greater
            unused_table_vals.append(sorted_table[j])
            j += 1
        elif input_val < table_val:                                      # Ordering::Less
            if unused_table_vals:
                permuted_table[i] = unused_table_vals.pop()
            else:
                unused_table_inds.append(i)
            i += 1
        else:                                                            # Ordering::Equal
            permuted_table[i] = sorted_table[j]
            i += 1
            j += 1
    unused_table_vals.extend(sorted_table[j:n])                          # :119
    unused_table_inds.extend(range(i, n))                                # :120
    assert len(unused_table_inds) == len(unused_table_vals)              # zip_eq, :122
    for ind, val in zip(unused_table_inds, unused_table_vals):
        permuted_table[ind] = val
    return sorted_inputs, permuted_table


def eval_lookups(local_in, next_in, next_table):
    """the two constraints of eval_lookups on one pair of rows -> (constraint, constraint_last_row), each BEFORE its filter:
    (next_in - local_in)(next_in - next_table) on every row, next_in - next_table where the next row is the first"""
    diff_input_prev = (next_in - local_in) % P
    diff_input_table = (next_in - next_table) % P
    return diff_input_prev * diff_input_table % P, diff_input_table


def lookup_rows_vanish(permuted_inputs, permuted_table):
    """per row i (the next row is i + 1 mod n) whether both constraints vanish under their filters"""
    n = len(permuted_inputs)
    out = []
    for i in range(n):
        nx = (i + 1) % n
        every, last = eval_lookups(permuted_inputs[i], permuted_inputs[nx], permuted_table[nx])
        out.append(every == 0 and (i != n - 1 or last == 0))
    return out
