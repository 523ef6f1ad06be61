"""A plain Python-integer model of the sigma polynomials of build() (no tests here).

What csrc/sigma.hip computes (k_sigma_keys, a 64-bit radix sort, k_sigma_heads, a max-scan, k_sigma_values), written from the reference, in
the reference's order:
  plonk/permutation_argument.rs:89-104    Forest::wire_partition          `for row, for column`, every wire appended to the list of its class
  plonk/permutation_argument.rs:135-156   WirePartition::get_sigma_map    inside a list every wire maps to the next one, the last to the first
  plonk/permutation_argument.rs:112-131   WirePartition::get_sigma_polys  sigma[column][row] = k_is[next.column] * subgroup[next.row]
The class of a wire is whatever id the caller gives it (the reference: the representative its union-find forest assigns): any u64, equal ids
= wires constrained equal.  A dict of lists and no sort: the kernels sort, the model must not share that idea.
Only Python `int` arithmetic mod P: no numpy on field values, no oracle, no product library.
"""
from vanishing_model import NUM_ROUTED, P, primitive_root


def _columns(a):
    return [[int(v) for v in (col.tolist() if hasattr(col, "tolist") else col)] for col in a]


def subgroup(lg_n):
    """F::two_adic_subgroup(lg_n): 1, w, w^2, ... (circuit_builder.rs:1003)"""
    w, x, out = primitive_root(lg_n), 1, []
    for _ in range(1 << lg_n):
        out.append(x)
        x = x * w % P
    return out


def wire_partition(classes, lg_n):
    """Forest::wire_partition (:89-104): class id -> its wires (row, column), in the order `for row, for column` meets them"""
    classes = _columns(classes)
    n = 1 << lg_n
    assert len(classes) == NUM_ROUTED and all(len(c) == n for c in classes)
    partition = {}
    for row in range(n):
        for column in range(NUM_ROUTED):
            partition.setdefault(classes[column][row], []).append((row, column))
    return partition


def sigma_map(partition):
    """WirePartition::get_sigma_map (:135-156) before it flattens the wires: wire -> its neighbour, the next wire of its subset, the last
    one looping around, a wire with a subset to itself its own neighbour"""
    neighbors = {}
    for subset in partition.values():
        if len(subset) == 1:
            neighbors[subset[0]] = subset[0]
        else:
            neighbors.update(zip(subset, subset[1:] + subset[:1]))      # subset[i] -> subset[(i + 1) % len]
    return neighbors


def sigma_values(classes, k_is, lg_n):
    """-> [80][n] canonical VALUES on H of the sigma polynomials (WirePartition::get_sigma_polys, :112-131).  `classes` [80][n] any u64,
    `k_is` the 80 coset shifts."""
    k_is = [int(k) % P for k in k_is]
    assert len(k_is) == NUM_ROUTED
    n, xs = 1 << lg_n, subgroup(lg_n)
    neighbors = sigma_map(wire_partition(classes, lg_n))
    assert len(neighbors) == NUM_ROUTED * n
    sigma = [[None] * n for _ in range(NUM_ROUTED)]
    for (row, column), (nrow, ncol) in neighbors.items():           # every wire once, whatever the order
        sigma[column][row] = k_is[ncol] * xs[nrow] % P
    return sigma


def wires_of_sigma(sigma, k_is, lg_n):
    """the wire (row, column) every sigma value k_is[column] * w^row names; raises if a value names none or the cosets k H are not disjoint"""
    sigma, k_is = _columns(sigma), [int(k) % P for k in k_is]
    n, xs = 1 << lg_n, subgroup(lg_n)
    assert len(sigma) == NUM_ROUTED and len(k_is) == NUM_ROUTED and all(len(c) == n for c in sigma)
    wire_at = {k_is[column] * xs[row] % P: (row, column) for column in range(NUM_ROUTED) for row in range(n)}
    assert len(wire_at) == NUM_ROUTED * n, "the cosets k_is[j] H are not disjoint"
    return {(row, column): wire_at[sigma[column][row]] for column in range(NUM_ROUTED) for row in range(n)}


def cycles_of_sigma(sigma, k_is, lg_n):
    """the cycles of a sigma matrix, each from its first wire in (row, column) order and in the order sigma walks it, the cycles ordered by
    that first wire; raises if sigma is no permutation of the wires"""
    nxt = wires_of_sigma(sigma, k_is, lg_n)
    assert len(set(nxt.values())) == len(nxt), "sigma is not a bijection on the wires"
    seen, cycles = set(), []
    for row in range(1 << lg_n):
        for column in range(NUM_ROUTED):
            if (row, column) in seen:
                continue
            cycle, w = [], (row, column)
            while w not in seen:
                seen.add(w)
                cycle.append(w)
                w = nxt[w]
            cycles.append(cycle)
    return cycles


def classes_from_sigma(sigma, k_is, lg_n):
    """-> classes [80][n] (Python ints): the partition a sigma matrix encodes, the id of a class = row * 80 + column of the first wire of its
    cycle in (row, column) order.  sigma_values of the result is `sigma` again exactly when every cycle walks its wires in that order."""
    classes = [[0] * (1 << lg_n) for _ in range(NUM_ROUTED)]
    for cycle in cycles_of_sigma(sigma, k_is, lg_n):
        ident = cycle[0][0] * NUM_ROUTED + cycle[0][1]
        for row, column in cycle:
            classes[column][row] = ident
    return classes
