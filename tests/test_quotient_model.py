"""The five quotient launches (csrc/prover_kernels.cuh: k_quotient<false>, k_quotient<true>, k_quotient_lookup,
k_quotient_random_access, k_quotient_ext_arith) point by point against the Python-integer model (tests/vanishing_model.py, itself pinned
by tests/test_vanishing_model.py).

In a proof the kernels' operands are LDE values of a satisfying witness: random-looking, so an operand such as 0, p - 1 or 2^32 reaches a
multiplier with probability 2^-32.  Here the inputs are chosen on the LDE coset itself: the points i = k (mod 8) of 7 <w_N> are the
coset 7 w_N^k <w_n> of H_n, on which a polynomial of degree < n takes any n values, so every input column is interpolated through chosen
edge values there.  One point in eight then carries edge operands in EVERY column (and in pairs, triples, ... of them: all-0, all-1 and
all-(p - 1) rows among them); the other seven carry the random-looking values of the same polynomials.  quotient_polys runs exactly
gl_prove's launches on these (non-satisfying) inputs; its result, taken back to values, is compared with the model at all 2N words."""
import numpy as np
import pytest

import ext_gate_circuits as egc
import vanishing_model as vm

pytestmark = pytest.mark.gpu
P = vm.P
EDGES = [0, 1, 2, P - 1, P - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, P - 2**32]
RESIDUES = [0, 5]
# S-box inputs whose 7th power takes the cold block of the Goldilocks product (gl64_gfx950.cuh glx_mul<false> / glx_mul3<false>: subtract EPS
# without a carry, tests/test_sbox_cold_paths.py): x x for 2^48, x^2 x^2 for 2^24, x^3 x^4 for 2^14
SBOX_COLD = [2**48, 2**24, 2**14]


def bit_wires(desc):
    """the wire columns some gate of the circuit reads as a bit: the PoseidonGate's swap, the limbs of BaseSumGate<2>, the power bits of the
    ExponentiationGate, the index bits of the RandomAccessGate"""
    cols = set()
    for g in range(desc.num_gates):
        t = desc.gate_types[g]
        if t == vm.POSEIDON:
            cols.add(24)
        elif t == vm.BASE_SUM:
            cols.update(range(1, 64))
        elif t == vm.EXPONENTIATION:
            cols.update(range(1, 67))
        elif t == vm.RANDOM_ACCESS:
            bits = desc.gate_params[g]
            copies, extra = vm.random_access_layout(bits)
            first = (2 + (1 << bits)) * copies + extra
            cols.update(range(first, first + copies * bits))
    return sorted(cols)


def edge_targets(rng, ncols, n, special=None):
    """[ncols][n] target values: rows 0, 1, 2 hold 0, 1, p - 1 in every column, the others seeded draws from EDGES; `special` maps a column
    to extra values that half of its draws come from"""
    t = np.array(EDGES, dtype=np.uint64)[rng.integers(0, len(EDGES), size=(ncols, n))]
    for col, extra in (special or {}).items():
        pick = np.array(extra, dtype=np.uint64)[rng.integers(0, len(extra), size=n)]
        t[col] = np.where(rng.integers(0, 2, size=n) == 1, pick, t[col])
    for r, v in enumerate([0, 1, P - 1][:n]):
        t[:, r] = v
    return t


def through_points(orc, targets, lg_n, k):
    """the value columns (on H_n) of the polynomials of degree < n that take `targets` on the LDE points i = k + 8 r"""
    shift = vm.COSET_SHIFT * pow(vm.primitive_root(lg_n + 3), k, P) % P
    return orc.fft(orc.coset_ifft(targets, shift))


CHALLENGES = {
    "random": None,
    "edges": dict(alphas=[P - 1, 2**32], betas=[P - 1, 1], gammas=[0, P - 1], pi_hash=[P - 1, 0, 1, 2**32],
                  deltas=[P - 1, 1, 0, P - 1, 2**32, P - 2**32, 2**32 - 1, 2]),
    "non-canonical": dict(alphas=[P + 3, 2**64 - 1], betas=[2**64 - 1, P + 3], gammas=[P + 3, P + 3], pi_hash=[P + 3, 2**64 - 1, P + 3, 2**64 - 1],
                          deltas=[P + 3, 2**64 - 1] * 4),
}


def challenge_set(name, rng):
    if CHALLENGES[name] is None:
        draw = lambda k: [int(v) for v in rng.integers(0, P, size=k, dtype=np.uint64)]
        return dict(alphas=draw(2), betas=draw(2), gammas=draw(2), pi_hash=draw(4), deltas=draw(8))
    return CHALLENGES[name]


def run_case(gpu, orc, desc, k, seed, kept_constants=None, sbox_cold=False):
    """steps 1-9 of one case: `desc` with every column free except `kept_constants` (the circuit's own constant columns, where the loader
    checks them); residue k.  sbox_cold (a circuit with the PoseidonGate): every S-box of the gate also meets the SBOX_COLD values -- in
    k_quotient<true> every S-box input but the first round's is a wire value, so the S-box input wire columns draw half of their targets
    from them; the first round reads inputs + deltas + RC[0], so rows 3, 4, 5 hold value - RC[0][i] in the inputs, swap 0 and deltas 0."""
    p, ctx = gpu
    rng = np.random.Generator(np.random.PCG64(seed))
    lg_n = desc.degree_bits
    n, N = 1 << lg_n, 8 << lg_n
    nlp, nc = desc.num_lookup_polys, desc.num_constants
    edge_points = np.arange(k, N, 8)
    assert len(edge_points) == n

    # 2. targets on the points i = k (mod 8); the selector columns also take the values the filters compare against
    selector_values = list(range(desc.num_gates)) + [vm.UNUSED_SELECTOR]
    t_cs = edge_targets(rng, nc + 80, n, {c: selector_values for c in range(desc.num_selectors)})
    bits = bit_wires(desc)
    special = {c: [0, 1] for c in bits}
    if sbox_cold:
        assert vm.POSEIDON in set(desc.gate_types[g] for g in range(desc.num_gates)) and n >= 6
        special.update({c: SBOX_COLD for c in vm.PSD_FULL_SBOX_WIRES + vm.PSD_PARTIAL_SBOX_WIRES})
    t_w = edge_targets(rng, 135, n, special)
    if sbox_cold:
        rc0 = vm._poseidon_tables()[0][0]
        for row, value in zip((3, 4, 5), SBOX_COLD):
            t_w[0:12, row] = [(value - rc0[i]) % P for i in range(12)]
            t_w[vm.PSD_WIRE_SWAP:vm.PSD_WIRE_DELTA + 4, row] = 0
    t_z = edge_targets(rng, 20 + 2 * nlp, n)
    # 3. interpolate and evaluate on H_n
    cs_values = through_points(orc, t_cs, lg_n, k)
    if kept_constants is not None:
        cs_values[:nc] = kept_constants
    # 4. the circuit, the batches, the launches, the inputs as the kernels read them
    cd = p.GenericCircuitData(desc, cs_values)
    wires_b = p.PolynomialBatch.from_values(list(through_points(orc, t_w, lg_n, k)), desc.rate_bits, False, desc.cap_height)
    zs_b = p.PolynomialBatch.from_values(list(through_points(orc, t_z, lg_n, k)), desc.rate_bits, False, desc.cap_height)
    cs, wires, zs = cd.constants_sigmas_batch.lde_values(), wires_b.lde_values(), zs_b.lde_values()
    # 5. the construction: one point in eight carries its intended edge value in every free column
    first_free = nc if kept_constants is not None else 0
    assert (cs[first_free:, edge_points] == t_cs[first_free:]).all() and (wires[:, edge_points] == t_w).all() and (zs[:, edge_points] == t_z).all()
    first_round = [(value - c) % P for value in SBOX_COLD for c in vm._poseidon_tables()[0][0]] if sbox_cold else []
    for arr in (cs[first_free:], wires, zs):
        allowed = EDGES + selector_values + (SBOX_COLD + first_round if arr is wires else [])
        assert np.isin(arr[:, edge_points], np.array(allowed, dtype=np.uint64)).all()
        assert (arr[:, edge_points[0]] == 0).all() and (arr[:, edge_points[1]] == 1).all() and (arr[:, edge_points[2]] == P - 1).all()
        others = np.delete(arr, edge_points, axis=1)
        assert np.isin(others, np.array(EDGES, dtype=np.uint64)).mean() < 0.01          # the other seven in eight are the random part
    for c in bits:
        assert {0, 1} <= set(int(v) for v in wires[c, edge_points])
    if sbox_cold:
        # each value sits at an edge point of a full-round and of a partial-round S-box input wire, and in front of the first round
        rc0 = vm._poseidon_tables()[0][0]
        for row, value in zip((3, 4, 5), SBOX_COLD):
            assert (wires[vm.PSD_FULL_SBOX_WIRES][:, edge_points] == value).any() and (wires[vm.PSD_PARTIAL_SBOX_WIRES][:, edge_points] == value).any()
            at = edge_points[row]
            assert all((int(wires[i, at]) + int(wires[vm.PSD_WIRE_DELTA + i, at]) * (1 if i < 4 else 0) + rc0[i]) % P == value for i in range(12))
            assert not wires[vm.PSD_WIRE_SWAP:vm.PSD_WIRE_DELTA + 4, at].any()

    def launch(ch):
        q_b = cd.quotient_polys(wires_b, zs_b, ch["pi_hash"], ch["betas"], ch["gammas"], ch["alphas"], deltas=ch["deltas"] if nlp else None)
        return q_b.polynomials

    results = {}
    for name in CHALLENGES:
        ch = challenge_set(name, rng)
        got = launch(ch)
        if name == "non-canonical":                     # (c) equals the call with the canonical residues, which is compared below
            canonical = {key: [v % P for v in vals] for key, vals in ch.items()}
            assert (got == launch(canonical)).all(), "non-canonical challenges and their residues give different quotients"
        # 6. the model on the read-back integers  7. the chunks back to values  8. all 2N words
        want = np.array(vm.vanishing_over_z_h(desc, cs, wires, zs, ch["pi_hash"], ch["betas"], ch["gammas"], ch["alphas"],
                                              ch["deltas"] if nlp else None), dtype=np.uint64)
        values = orc.coset_fft(got.reshape(2, N), 7)
        bad = np.argwhere(values != want)
        # 9.
        assert not len(bad), "challenges %r: %d of %d words differ; first: %s" % (name, len(bad), 2 * N, ", ".join(
            "point %d (i mod 8 = %d, %s point) output of challenge %d" % (i, i % 8, "edge" if i % 8 == k else "random", b) for b, i in bad[:6]))
        results[name] = values
    return results, (cs, wires, zs)


# ------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("k", RESIDUES)
@pytest.mark.parametrize("lg_n", [4, 6])
def test_main_and_extension_gate_launches_on_the_chained_circuit(gpu, orc, lg_n, k):
    # k_quotient<false> (Noop, Constant, PublicInput, Arithmetic; the permutation terms with the running x7) and k_quotient_ext_arith (the four
    # extension gates), two selector groups; N = 128 is under one block of 256, N = 512 is two.  All of constants || sigmas free.
    desc = egc.Chained(seed=1, min_degree_bits=lg_n).circuit.desc
    assert desc.degree_bits == lg_n and desc.num_selectors == 2
    assert {vm.ARITHMETIC, vm.ARITHMETIC_EXT, vm.MUL_EXT, vm.REDUCING, vm.REDUCING_EXT} <= set(desc.gate_types[g] for g in range(desc.num_gates))
    run_case(gpu, orc, desc, k, seed=100 * lg_n + k)


@pytest.mark.parametrize("k", RESIDUES)
def test_main_poseidon_and_lookup_launches_on_the_circuit_with_every_oracle_gate(gpu, orc, k):
    # oracle kind 15 at its smallest (bits = 1): k_quotient<false> (BaseSum, Exponentiation, Arithmetic, ...), k_quotient<true> and
    # k_quotient_lookup with two tables; three selector groups.  The constants are the circuit's own (the loader reads the lookup rows from
    # the lookup selector columns); sigmas, wires, Z, partial products and lookup polynomials free.  The circuit with the PoseidonGate: its
    # S-box input wires also carry the values whose 7th power takes the cold block of the Goldilocks product (run_case sbox_cold).
    oc = orc.circuit_of_kind(15, 1, threads=4)
    desc = oc.product_desc()
    types = set(desc.gate_types[g] for g in range(desc.num_gates))
    assert {vm.POSEIDON, vm.BASE_SUM, vm.EXPONENTIATION, vm.LOOKUP, vm.LOOKUP_TABLE} <= types and desc.num_luts == 2 and desc.num_lookup_polys == 7
    run_case(gpu, orc, desc, k, seed=1500 + k, kept_constants=oc.constants_sigmas()[:desc.num_constants], sbox_cold=True)


@pytest.mark.parametrize("k", RESIDUES)
@pytest.mark.parametrize("bits", [1, 2, 3, 4, 5, 6])
def test_random_access_launch_for_every_index_width(gpu, orc, bits, k):
    # oracle kind 16: one glq_random_access_gate<BITS> instantiation each (20 / 13 / 8 / 4 / 2 / 1 copies, with and without extra constants)
    desc = orc.circuit_of_kind(16, bits, threads=4).product_desc()
    assert [desc.gate_params[g] for g in range(desc.num_gates) if desc.gate_types[g] == vm.RANDOM_ACCESS] == [bits]
    run_case(gpu, orc, desc, k, seed=1600 + 10 * bits + k)


@pytest.mark.parametrize("k", RESIDUES)
def test_coset_shifts_that_are_not_powers_of_seven(gpu, orc, k):
    # the general k_is path of k_quotient<false> (beta x k_j by one product per wire instead of the running x7), which no proved circuit
    # takes: the m = 1 matmul description with k_is[j] = 3^(j + 1), everything free
    desc = orc.circuit(1, threads=4).product_desc()
    sevens = [pow(7, j, P) for j in range(80)]
    assert [int(desc.k_is[j]) for j in range(80)] == sevens
    for j in range(80):
        desc.k_is[j] = pow(3, j + 1, P)
    assert len({int(desc.k_is[j]) for j in range(80)}) == 80 and all(int(desc.k_is[j]) != sevens[j] for j in range(80))
    results, (cs, wires, zs) = run_case(gpu, orc, desc, k, seed=1700 + k)
    # and the shifts matter to the result: the model with the usual 7^j disagrees with what the launches gave
    for j in range(80):
        desc.k_is[j] = sevens[j]
    ch = CHALLENGES["edges"]
    usual = np.array(vm.vanishing_over_z_h(desc, cs, wires, zs, ch["pi_hash"], ch["betas"], ch["gammas"], ch["alphas"]), dtype=np.uint64)
    assert (usual != results["edges"]).any()
