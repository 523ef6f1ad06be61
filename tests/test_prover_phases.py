"""The prover's launches on either side of the quotient (csrc/prover_kernels.cuh), by value against the Python-integer model
(tests/prover_phase_model.py, itself pinned by tests/test_prover_phase_model.py):
  gl_partial_products           k_pp_chunk_terms, k_pp_chunk_products, k_z_segment_products, k_z_segment_scan, k_z_finalize
  gl_partial_products_lookups   k_lookup_inverses, k_lookup_scan
  gl_open_at; inside gl_prove   k_eval_at_ext; k_ext_powers2 + k_eval_list_with_powers
  gl_fri_combine                k_fri_combine, k_div_linear_heads, k_div_linear_carries, k_div_linear_apply
  gl_fri_fold                   k_fri_fold

In a proof the challenges come out of the transcript and the polynomials out of a satisfying witness: an operand such as 0, p - 1 or 2^32,
a zeta in the base field, a fri_alpha of 0 or 1 reach these kernels with probability 2^-32 or less, and n is whatever the circuit has.
Here the phase API is driven with chosen challenges (seeded random, edge, non-canonical), with wire / sigma values and polynomial
coefficients drawn from EDGES, and with n at the kernels' branch points (a block, a scan segment, a division segment, the unrolled loop of
the openings).  Every word is compared.  The inputs do not satisfy any circuit: the kernels have to produce these values all the same.
No input cell is omitted or repaired: the model's zero checks pass on the committed seeds."""
import numpy as np
import pytest

import prover_phase_model as pm
from oracle_lib import m1_desc
from proof_parser import ParsedProof
from test_prover_phase_model import ZETAS, lookup_rows, pairs
from test_quotient_model import EDGES, edge_targets

pytestmark = pytest.mark.gpu
P = pm.P
U64 = np.uint64
SETS = ["random", "edges", "non-canonical"]
UNIFORM_ROWS = {0: "the all-0 row", 1: "the all-1 row", 2: "the all-(p - 1) row"}


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def draw(rng, k):
    return [int(v) for v in rng.integers(0, P, size=k, dtype=U64)]


def canonical(ch):
    return {key: [v % P for v in vals] for key, vals in ch.items()}


def edge_columns(seed, ncols, n):
    return edge_targets(rng_of(seed), ncols, n)


def first_differences(got, want, describe, limit=6):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return "%d of %d words differ; first: %s" % (len(bad), np.asarray(want).size, "; ".join(describe(*(int(v) for v in b)) for b in bad[:limit]))


# ------------------------------------------------------------------------------- the permutation argument
# betas / gammas.  edges: no w + beta sigma + gamma vanishes for any w, sigma in EDGES (40 of the 196 pairs of edge values have this
# property; (p - 1, 0) and the like do not).  non-canonical: P + 1, P + 3 with 2^64 - 2, 2^64 - 1, whose residues 1, 3 with 2^32 - 3,
# 2^32 - 2 have the same property.
PERM_CHALLENGES = {
    "random": None,
    "edges": dict(betas=[P - 1, 2**32], gammas=[5, 2**63 - 1]),
    "non-canonical": dict(betas=[P + 1, P + 3], gammas=[2**64 - 2, 2**64 - 1]),
    "beta = 0": dict(betas=[0, 2**32 + 1], gammas=[2**32 + 1, 5]),
}
ZS_COLUMNS = ["Z of challenge 0", "Z of challenge 1"] + ["partial product %d of challenge %d" % (c, a) for a in range(2) for c in range(9)]


def perm_challenges(name, seed):
    if PERM_CHALLENGES[name] is None:
        rng = rng_of(seed)
        return dict(betas=draw(rng, 2), gammas=draw(rng, 2))
    ch = PERM_CHALLENGES[name]
    assert all((w + b * s + g) % P for b, g in zip(ch["betas"], ch["gammas"]) for w in EDGES for s in EDGES)      # the property claimed above
    return ch


def describe_zs(col, row):
    return "%s, row %d (%s)" % (ZS_COLUMNS[col] if col < 20 else "lookup polynomial %d of challenge %d" % ((col - 20) % 7, (col - 20) // 7), row,
                                UNIFORM_ROWS.get(row, "edge draws"))


def perm_inputs(d, seed, name, sigmas=None):
    """(wire values [135][n], constants || sigmas values, challenges): edge draws, rows 0, 1, 2 all-0, all-1, all-(p - 1)"""
    n = 1 << d.degree_bits
    wires = edge_columns(seed, 135, n)
    cs = edge_columns(seed + 1, d.num_constants + 80, n)
    if sigmas is not None:
        cs[d.num_constants:] = sigmas
    return wires, cs, perm_challenges(name, seed + 2)


def run_partial_products(gpu, orc, d, seed, name, sigmas=None):
    """gl_partial_products on edge wire and sigma VALUES (the kernels read values on H: no interpolation); -> (the 20 value columns, wires,
    sigmas, challenges)"""
    p, ctx = gpu
    wires, cs, ch = perm_inputs(d, seed, name, sigmas)
    cd = p.GenericCircuitData(d, cs, ctx)
    d_w = ctx.alloc(wires.nbytes).upload(wires)
    launch = lambda c: orc.fft(cd.partial_products(d_w.ptr, c["betas"], c["gammas"]).polynomials)
    got = launch(ch)
    if name == "non-canonical":
        assert (got == launch(canonical(ch))).all(), "non-canonical challenges and their residues give different Z / partial products"
    assert (d_w.download(wires.shape) == wires).all(), "the wire matrix on the device changed"
    d_w.free()
    return got, wires, cs[d.num_constants:], ch


@pytest.mark.parametrize("name", SETS + ["beta = 0"])
@pytest.mark.parametrize("lg_n", [4, 11, 12])
def test_partial_products_and_z(gpu, orc, lg_n, name):
    # n = 16: under one block, the i < n guards live; 2048: exactly one scan segment (GLP_SEG); 4096: two segments, seg_excl is used
    d = m1_desc(orc, lg_n)
    k_is = [int(d.k_is[j]) for j in range(80)]
    assert k_is == [pow(7, j, P) for j in range(80)]                # the running x7 of k_pp_chunk_terms
    got, wires, sigmas, ch = run_partial_products(gpu, orc, d, 6000 + 10 * lg_n, name)
    want = np.array(pm.partial_products(wires, sigmas, k_is, ch["betas"], ch["gammas"], lg_n), dtype=U64)      # raises on a zero factor
    assert (got == want).all(), "challenges %r: %s" % (name, first_differences(got, want, describe_zs))
    if name == "beta = 0":                                          # every quotient of challenge 0 is (w + gamma) / (w + gamma)
        assert (got[0] == 1).all() and (got[2:11] == 1).all() and not (got[1] == 1).all()


@pytest.mark.parametrize("name", SETS)
def test_partial_products_with_coset_shifts_that_are_not_powers_of_seven(gpu, orc, name):
    # k_is_powers_of_7 = 0: beta x k_j by one product per wire
    d = m1_desc(orc, 4)
    k_is = [pow(3, j + 1, P) for j in range(80)]
    for j in range(80):
        d.k_is[j] = k_is[j]
    got, wires, sigmas, ch = run_partial_products(gpu, orc, d, 6100, name)
    want = np.array(pm.partial_products(wires, sigmas, k_is, ch["betas"], ch["gammas"], 4), dtype=U64)
    assert (got == want).all(), "challenges %r: %s" % (name, first_differences(got, want, describe_zs))
    usual = pm.partial_products(wires, sigmas, [pow(7, j, P) for j in range(80)], ch["betas"], ch["gammas"], 4)
    assert (np.array(usual, dtype=U64) != got).any()                # and the shifts matter to the result


@pytest.mark.parametrize("name", SETS)
def test_identity_permutation_gives_constant_one_over_four_segments(gpu, orc, name):
    # sigma_j = k_j x: numerator = denominator on every cell, so Z and all partial products are 1 on all 8192 rows, whatever the wires
    lg_n, n = 13, 8192
    d = m1_desc(orc, lg_n)
    g, x, xs = pm.primitive_root(lg_n), 1, []
    for _ in range(n):
        xs.append(x)
        x = x * g % P
    sigmas = np.array([[int(d.k_is[j]) * x % P for x in xs] for j in range(80)], dtype=U64)
    got, wires, _, ch = run_partial_products(gpu, orc, d, 6200, name, sigmas=sigmas)
    c = canonical(ch)
    for a in range(2):                                              # no factor vanishes (the quotients are 1 only then)
        for j in range(80):
            col, sig = wires[j].tolist(), sigmas[j].tolist()
            assert all((w + c["betas"][a] * s + c["gammas"][a]) % P for w, s in zip(col, sig)), (a, j)
    assert (got == 1).all(), "challenges %r: %s" % (name, first_differences(got, np.ones_like(got), describe_zs))


# ------------------------------------------------------------------------------- the lookup polynomials
# the 8 lookup challenges, per challenge (A, B, Alpha, Delta).  Alpha - (inp + A out) must not vanish; with out = 0 that rules out every
# Alpha in EDGES, so the edge set takes Alpha next to an edge: (A, Alpha) = (p - 1, 5) and (2^32, 2^63 + 1) leave no zero for any inp, out
# in EDGES, and so do the residues (1, 5) and (2^32 - 2, 5) of the non-canonical (P + 1, P + 5), (2^64 - 1, P + 5).
LOOKUP_DELTAS = {
    "random": None,
    "edges": [P - 1, P - 1, 5, P - 1, 2**32, 0, 2**63 + 1, 2**32],
    "non-canonical": [P + 1, 2**64 - 1, P + 5, P + 3, 2**64 - 1, P + 3, P + 5, 2**64 - 1],
}


@pytest.mark.parametrize("name", SETS)
def test_lookup_polynomials_on_the_circuit_with_two_tables(gpu, orc, name):
    # oracle kind 15 at its smallest: n = 32, LookupGate rows 5 and 17, LookupTableGate rows 6..15 and 18..27; the circuit's own constants
    # (the loader reads the lookup rows from the lookup selector columns), sigmas and all 135 wires free edge values
    p, ctx = gpu
    oc = orc.circuit_of_kind(15, 1, threads=4)
    d = oc.product_desc()
    n = 1 << d.degree_bits
    assert n == 32 and d.num_luts == 2 and d.num_lookup_polys == 7 and lookup_rows(d) == [(5, 6, 15), (17, 18, 27)]
    cs = oc.constants_sigmas()
    cs[d.num_constants:] = edge_columns(6301, 80, n)
    wires = edge_columns(6300, 135, n)
    cd = p.GenericCircuitData(d, cs, ctx)
    d_w = ctx.alloc(wires.nbytes).upload(wires)
    ch = dict(perm_challenges(name, 6302))
    ch["deltas"] = draw(rng_of(6303), 8) if LOOKUP_DELTAS[name] is None else LOOKUP_DELTAS[name]
    if LOOKUP_DELTAS[name] is not None:                             # the property claimed above
        assert all((ch["deltas"][4 * c + 2] - (i + ch["deltas"][4 * c] * o)) % P for c in range(2) for i in EDGES for o in EDGES)
    launch = lambda c: orc.fft(cd.partial_products(d_w.ptr, c["betas"], c["gammas"], deltas=c["deltas"]).polynomials)
    got = launch(ch)
    if name == "non-canonical":
        assert (got == launch(canonical(ch))).all(), "non-canonical challenges and their residues give different lookup polynomials"
    assert (d_w.download(wires.shape) == wires).all(), "the wire matrix on the device changed"
    d_w.free()
    want = pm.partial_products(wires, cs[d.num_constants:], [int(d.k_is[j]) for j in range(80)], ch["betas"], ch["gammas"], d.degree_bits)
    want = np.array(want + pm.lookup_polys(wires, lookup_rows(d), ch["deltas"]), dtype=U64)                  # raises on a zero denominator
    assert got.shape == want.shape == (34, n)
    assert (got == want).all(), "challenges %r: %s" % (name, first_differences(got, want, describe_zs))
    outside = [r for r in range(n) if not (5 <= r <= 15 or 17 <= r <= 27)]
    assert (got[20:, outside] == 0).all() and (got[20:, 5:16] != 0).any()


# ------------------------------------------------------------------------------- open_at
@pytest.mark.parametrize("n", [2, 16, 256, 512, 4096])
def test_open_at(gpu, n):
    # k_eval_at_ext: 256 strips of ceil(n / 256) coefficients; n = 2 and 16 leave most strips empty, 256 is one coefficient per strip
    p, ctx = gpu
    coeffs = np.array(EDGES, dtype=U64)[rng_of(6400 + n).integers(0, len(EDGES), size=(8, n))]
    coeffs[0], coeffs[1], coeffs[2] = 0, 1, P - 1                   # the all-0, all-1 and all-(p - 1) polynomials; the others edge draws
    b = p.PolynomialBatch.from_coeffs(list(coeffs), 3, False, 4, ctx=ctx)
    assert (b.polynomials == coeffs).all()
    for z in ZETAS:
        got = b.open_at(z)
        want = [pm.eval_ext(c, z) for c in coeffs]
        assert pairs(got.reshape(-1)) == want, "z = (%#x, %#x): %s" % (z + (first_differences(got, np.array(want, dtype=U64), lambda c, h: "column %d, half %d" % (c, h)),))
        if z[0] >= P or z[1] >= P:
            assert (got == b.open_at((z[0] % P, z[1] % P))).all(), "a non-canonical point and its residue open differently"
        assert (b.open_at(z, first_col=3, num_cols=4) == got[3:7]).all() and b.open_at(z, first_col=7).shape == (1, 2)
    assert any(z[0] >= P for z in ZETAS)


# ------------------------------------------------------------------------------- the openings inside gl_prove
@pytest.mark.parametrize("lg_n", [4, 9, 11])
def test_openings_of_a_proof(gpu, orc, lg_n):
    # k_ext_powers2 + k_eval_list_with_powers: thread t sums i = t, t + 256, ..., four at a time while i + 768 < n.  n = 16 and 512: the
    # tail loop only, 1 and 2 iterations; n = 2048: two unrolled iterations and no tail.  Edge COEFFICIENTS in constants || sigmas and the
    # wires; the witness does not satisfy the circuit and the proof is not verified.  zeta is the proof's own.
    p, ctx = gpu
    n = 1 << lg_n
    d = m1_desc(orc, lg_n)
    ctx.capture_intermediates(True)
    cs_c, wires_c = edge_columns(6500 + lg_n, d.num_constants + 80, n), edge_columns(6600 + lg_n, 135, n)
    cd = p.GenericCircuitData(d, orc.fft(cs_c), ctx)
    assert (cd.constants_sigmas_batch.polynomials == cs_c).all()
    proof = cd.prove(orc.fft(wires_c), np.arange(1, 1 + d.num_public_inputs, dtype=U64))
    pp = ParsedProof(d, proof.to_bytes())
    zeta = proof.challenges()["zeta"]
    g = pm.primitive_root(lg_n)
    gzeta = [zeta[0] * g % P, zeta[1] * g % P]
    zs_c, q_c = orc.ifft(proof.zs_partial_products()), proof.quotient_chunks()
    nc = d.num_constants
    for what, polys, point in (("constants", cs_c[:nc], zeta), ("sigmas", cs_c[nc:], zeta), ("wires", wires_c, zeta), ("zs", zs_c[:2], zeta),
                               ("zs_next", zs_c[:2], gzeta), ("pp", zs_c[2:20], zeta), ("quotient", q_c, zeta)):
        want, got = [pm.eval_ext(c, point) for c in polys], pairs(pp.openings[what])
        bad = [k for k in range(len(want)) if want[k] != got[k]]
        assert not bad, "%s at %s (%#x, %#x): openings %s differ (edge coefficients: %s)" % (
            what, "g zeta" if point is gzeta else "zeta", point[0], point[1], bad[:8], what in ("constants", "sigmas", "wires"))
    assert len(pp.openings["lookups"]) == 0


# ------------------------------------------------------------------------------- fri_combine + division, fri_fold
ALPHAS = {"0": (0, 0), "1": (1, 0), "X": (0, 1), "(p-1,p-1)": (P - 1, P - 1), "random": tuple(draw(rng_of(6700), 2)), "non-canonical": (2**64 - 1, P + 3)}
_oracles = {}


def four_oracles(gpu, orc, shape, rounds=0):
    """(circuit, its four committed batches, their coefficient columns) with edge coefficients in every column, once per shape: the m = 1
    description at n = 2^shape, or the kind-15 description (n = 32, its own constants, 14 lookup polynomials behind the 20) for "lookups" """
    p, ctx = gpu
    key = (shape, rounds)
    if key not in _oracles:
        if shape == "lookups":
            oc = orc.circuit_of_kind(15, 1, threads=4)
            d = oc.product_desc()
            assert d.degree_bits == 5 and d.num_fri_rounds == 0
            n = 32
            cs_v = oc.constants_sigmas()
            cs_v[d.num_constants:] = orc.fft(edge_columns(6801, 80, n))
        else:
            d, n = m1_desc(orc, shape, rounds), 1 << shape
            cs_v = orc.fft(edge_columns(6800 + shape, d.num_constants + 80, n))
        cd = p.GenericCircuitData(d, cs_v, ctx)
        coeffs = [orc.ifft(cs_v)] + [edge_columns(6810 + 10 * k + (0 if shape == "lookups" else shape), ncols, n)
                                     for k, ncols in enumerate((135, 20 + 2 * d.num_lookup_polys, 16))]
        batches = [cd.constants_sigmas_batch] + [p.PolynomialBatch.from_coeffs(list(c), 3, False, d.cap_height, ctx=ctx) for c in coeffs[1:]]
        for b, c in zip(batches, coeffs):
            assert (b.polynomials == c).all()
        _oracles[key] = (cd, batches, coeffs)
    return _oracles[key]


def describe_coefficient(k, half):
    return "coefficient %d, %s half" % (k, "imaginary" if half else "real")


@pytest.mark.parametrize("alpha", list(ALPHAS))
@pytest.mark.parametrize("shape", [4, 5, 6, 11, 12, "lookups"])
def test_fri_combine_and_division(gpu, orc, shape, alpha):
    # seg_len = 32 (or n): n = 16 and 32 are one segment, 64 two, 4096 is 128 segments in two blocks of k_div_linear_heads / _apply; no
    # reduction rounds, so final_poly() is the whole combined polynomial.  The reduction is modelled once per alpha, the division at every
    # zeta of the list (0 and base-field points among them).
    cd, batches, coeffs = four_oracles(gpu, orc, shape)
    d = cd.desc
    n, g, al = 1 << d.degree_bits, pm.primitive_root(d.degree_bits), ALPHAS[alpha]
    first, second = pm.opened_polys([pm._ints(c) for c in coeffs])
    assert len(first) == d.num_constants + 80 + 135 + 20 + 16 + 2 * d.num_lookup_polys and len(second) == 2 + 2 * d.num_lookup_polys
    f0, f1 = pm.reduce_polys_base(first, al), pm.reduce_polys_base(second, al)
    shift = (1, 0)
    for _ in range(len(second)):
        shift = pm._ext_mul(shift, pm._ext(al))
    for z in ZETAS:
        fri = cd.fri(batches, z, al)
        got = fri.final_poly()
        if alpha == "non-canonical" or z[0] >= P:
            again = cd.fri(batches, (z[0] % P, z[1] % P), (al[0] % P, al[1] % P))
            assert (got == again.final_poly()).all(), "non-canonical challenges and their residues combine differently"
            again.close()
        fri.close()
        q0 = pm.divide_by_linear(f0, z) + [(0, 0)]
        q1 = pm.divide_by_linear(f1, (z[0] * g % P, z[1] * g % P)) + [(0, 0)]
        want = np.array([tuple((s + b) % P for s, b in zip(pm._ext_mul(a, shift), b)) for a, b in zip(q0, q1)], dtype=U64)
        assert got.shape == (n, 2)
        assert (got == want).all(), "zeta (%#x, %#x), alpha %s: %s" % (z[0], z[1], alpha, first_differences(got, want, describe_coefficient))


def test_the_split_model_of_the_combine_test_is_the_models_combine_and_divide(gpu, orc):
    # the test above takes the model's reduction and division apart to reuse the reduction; put together they are combine_and_divide
    cd, batches, coeffs = four_oracles(gpu, orc, "lookups")
    z, al = ZETAS[6], ALPHAS["random"]
    fri = cd.fri(batches, z, al)
    want = pm.combine_and_divide(coeffs, z, pm.primitive_root(5), al)
    assert (fri.final_poly() == np.array(want, dtype=U64)).all()
    fri.close()


def test_fri_combine_over_1024_segments_of_64(gpu, orc):
    # n = 2^16: seg_len = n / 1024 = 64, the full width of k_div_linear_carries.  All but eight columns are the zero polynomial (read back
    # below); the eight are the first and the last column of each batch, which the model sums alone while the kernels sum all 255 + 2.
    p, ctx = gpu
    lg_n, n = 16, 1 << 16
    d = m1_desc(orc, lg_n)
    sizes = (d.num_constants + 80, 135, 20, 16)
    coeffs = []
    for k, ncols in enumerate(sizes):
        c = np.zeros((ncols, n), dtype=U64)
        c[[0, -1]] = edge_columns(6900 + k, 2, n)
        coeffs.append(c)
    cd = p.GenericCircuitData(d, orc.fft(coeffs[0]), ctx)
    batches = [cd.constants_sigmas_batch] + [p.PolynomialBatch.from_coeffs(list(c), 3, False, d.cap_height, ctx=ctx) for c in coeffs[1:]]
    for b, c in zip(batches, coeffs):
        back = b.polynomials
        assert (back[1:-1] == 0).all() and (back == c).all()
    groups = [[(col if j in (0, len(c) - 1) else None) for j, col in enumerate(c)] for c in coeffs]
    for z, al in ((ZETAS[6], ALPHAS["random"]), (ZETAS[7], ALPHAS["(p-1,p-1)"])):
        fri = cd.fri(batches, z, al)
        got = fri.final_poly()
        fri.close()
        want = np.array(pm.combine_and_divide(groups, z, pm.primitive_root(lg_n), al), dtype=U64)
        assert (got == want).all(), "zeta (%#x, %#x): %s" % (z[0], z[1], first_differences(got, want, describe_coefficient))
    for b in batches[1:]:
        b.close()
    cd.close()


BETAS = [(0, 0), (1, 0), (0, P - 1), tuple(draw(rng_of(7000), 2)), (P + 3, 2**64 - 1)]


@pytest.mark.parametrize("lg_n,rounds", [(5, 1), (12, 1), (12, 2)])
def test_fri_fold(gpu, orc, lg_n, rounds):
    # k_fri_fold, arity 16: n = 32 folds to 2 coefficients, 4096 to 256 (one block) and then to 16.  The committed caps are not
    # checked here: the whole-proof tests own the leaf layout.
    cd, batches, coeffs = four_oracles(gpu, orc, lg_n, rounds)
    z, al = ZETAS[7], ALPHAS["random"]
    combined = pm.combine_and_divide(coeffs, z, pm.primitive_root(lg_n), al)

    def folded(betas):
        fri = cd.fri(batches, z, al)
        for beta in betas:
            fri.commit_round()
            fri.fold(beta)
        out = fri.final_poly()
        fri.close()
        return out

    for k in range(len(BETAS)):
        betas = [BETAS[(k + r) % len(BETAS)] for r in range(rounds)]
        got = folded(betas)
        want = combined
        for beta in betas:
            want = pm.fold(want, 16, beta)
        want = np.array(want, dtype=U64)
        assert got.shape == (1 << (lg_n - 4 * rounds), 2)
        assert (got == want).all(), "betas %r: %s" % (betas, first_differences(got, want, describe_coefficient))
        if any(v >= P for beta in betas for v in beta):
            assert (got == folded([(b[0] % P, b[1] % P) for b in betas])).all(), "a non-canonical beta and its residue fold differently"
