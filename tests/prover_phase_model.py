"""A plain Python-integer model of the prover phases on either side of the quotient (no tests here).

What the launches of csrc/prover_kernels.cuh between the commitments compute, written from the reference, in the reference's order:
  plonk/prover.rs:332-416, util/partial_products.rs   partial_products   k_pp_chunk_terms, k_pp_chunk_products, k_z_segment_products,
                                                                         k_z_segment_scan, k_z_finalize
  plonk/prover.rs:425-572                             lookup_polys       k_lookup_inverses, k_lookup_scan
  plonk/proof.rs:306-344                              eval_ext           k_eval_at_ext; k_ext_powers2 + k_eval_list_with_powers
  fri/oracle.rs:162-219, util/reducing.rs:83-106,
  polynomial/division.rs:75-88                        combine_and_divide k_fri_combine, k_div_linear_heads / _carries / _apply
  fri/prover.rs:94-103, plonk_common.rs:116-128       fold               k_fri_fold
None of the kernels' reorderings is restated: one pow(x, P - 2, P) per denominator (remembered per operand, nothing batched), sequential
scans, sequential Horner division.
Only Python `int` arithmetic mod P: no numpy on field values, no oracle, no product library.  Every argument may be non-satisfying.
"""
import functools

from vanishing_model import CHUNK, NUM_CHUNKS, NUM_ROUTED, P, W, _ext_mul, _ints, primitive_root      # noqa: F401  (W, primitive_root: for the tests)
from vanishing_model import CH_A, CH_ALPHA, CH_B, CH_DELTA, LOOKUP_SLOTS, LOOKUP_TABLE_SLOTS

NUM_LOOKUP_POLYS = 7                    # RE and ceil(40 / 7) = 6 partial SLDC polynomials (prover.rs:436-446)


class UndefinedResult(ValueError):
    """the inputs leave the reference without a result to compare with"""


@functools.lru_cache(maxsize=1 << 16)
def _fermat(x):
    """x^(p - 2), remembered per operand: edge inputs repeat a few hundred denominators over millions of cells"""
    return pow(x, P - 2, P)


def _inv(x, *where):
    """one inversion per denominator; `where` = (format, arguments...) names the cell if it is zero"""
    x %= P
    if x == 0:
        raise UndefinedResult("zero denominator: %s (the reference panics: batch_multiplicative_inverse, \"Tried to invert zero\")" % (where[0] % where[1:]))
    return _fermat(x)


# ------------------------------------------------------------------------------- the permutation argument
def partial_products(wires, sigmas, k_is, betas, gammas, lg_n):
    """-> [20][n]: Z_0, Z_1, then the 9 partial products of challenge 0 and of challenge 1 (the column order of prover.rs:196-213, which
    is the order k_z_finalize writes).  `wires` [>= 80][n] and `sigmas` [80][n] are VALUES on H.
    wires_permutation_partial_products_and_zs (prover.rs:359-416): per row the 80 quotients (w + beta k_j x + gamma) / (w + beta sigma_j +
    gamma), their products over chunks of 8 (quotient_chunk_products, partial_products.rs:13-23), the running products from Z(x)
    (partial_products_and_z_gx, :27-37), the last of which is Z(g x).
    Raises UndefinedResult on a zero denominator factor (the reference panics) and on a zero numerator factor (every later Z would be 0
    and a comparison behind it says nothing)."""
    wires, sigmas = _ints(wires), _ints(sigmas)
    k_is, betas, gammas = ([int(v) % P for v in a] for a in (k_is, betas, gammas))
    n = 1 << lg_n
    assert len(sigmas) == NUM_ROUTED and len(k_is) == NUM_ROUTED and all(len(c) == n for c in wires[:NUM_ROUTED] + sigmas)
    g = primitive_root(lg_n)
    out = [[0] * n for _ in range(2 + 2 * (NUM_CHUNKS - 1))]
    for a in range(2):
        beta, gamma = betas[a], gammas[a]
        z_x, x = 1, 1
        for i in range(n):
            out[a][i] = z_x
            acc = z_x
            for c in range(NUM_CHUNKS):
                for j in range(CHUNK * c, CHUNK * (c + 1)):
                    num = (wires[j][i] + beta * (k_is[j] * x % P) + gamma) % P
                    den = (wires[j][i] + beta * sigmas[j][i] + gamma) % P
                    if num == 0:
                        raise UndefinedResult("zero numerator factor: challenge %d, row %d, wire %d" % (a, i, j))
                    acc = acc * (num * _inv(den, "challenge %d, row %d, wire %d", a, i, j) % P) % P
                if c < NUM_CHUNKS - 1:
                    out[2 + (NUM_CHUNKS - 1) * a + c][i] = acc
            z_x = acc                                   # Z(g x)
            x = x * g % P
    return out


# ------------------------------------------------------------------------------- the lookup polynomials
def lookup_polys(wires, rows, deltas):
    """-> [2 * 7][n]: per challenge RE and the six partial SLDC polynomials (compute_lookup_polys, prover.rs:425-541; the two challenges
    one after the other, :544-572).  `wires` [135][n] values, `rows` one (last_lu_row, last_lut_row, first_lut_row) per table in the
    order of ProverOnlyCircuitData::lookup_rows, `deltas` the 8 lookup challenges.  Raises UndefinedResult on a zero alpha - (inp + a out)."""
    wires = _ints(wires)
    deltas = [int(v) % P for v in deltas]
    n = len(wires[0])
    lu_degree = 8 - 1                                               # max_quotient_degree_factor - 1
    num_partial = -(-LOOKUP_SLOTS // lu_degree)
    lut_degree = -(-LOOKUP_TABLE_SLOTS // num_partial)
    assert num_partial + 1 == NUM_LOOKUP_POLYS
    out = []
    for c in range(2):
        d = deltas[4 * c:4 * c + 4]
        polys = [[0] * n for _ in range(num_partial + 1)]
        for last_lu_row, last_lut_row, first_lut_row in rows:
            for row in range(first_lut_row, last_lut_row - 1, -1):                  # partial Sums and RE
                inp = [wires[3 * s][row] for s in range(LOOKUP_TABLE_SLOTS)]         # lookup_table.rs:55-67
                outv = [wires[3 * s + 1][row] for s in range(LOOKUP_TABLE_SLOTS)]
                mult = [wires[3 * s + 2][row] for s in range(LOOKUP_TABLE_SLOTS)]
                inverses = [_inv(d[CH_ALPHA] - (inp[s] + d[CH_A] * outv[s]), "challenge %d, table row %d, slot %d", c, row, s)
                            for s in range(LOOKUP_TABLE_SLOTS)]
                re = polys[0][row + 1]
                for s in range(LOOKUP_TABLE_SLOTS):
                    re = (re * d[CH_DELTA] + inp[s] + d[CH_B] * outv[s]) % P
                polys[0][row] = re
                for slot in range(num_partial):
                    acc = polys[slot][row] if slot else polys[num_partial][row + 1]
                    for s in range(slot * lut_degree, min((slot + 1) * lut_degree, LOOKUP_TABLE_SLOTS)):
                        acc = (acc + mult[s] * inverses[s]) % P
                    polys[slot + 1][row] = acc
            for row in range(last_lut_row - 1, last_lu_row - 1, -1):                # partial LDCs
                inverses = [_inv(d[CH_ALPHA] - (wires[2 * s][row] + d[CH_A] * wires[2 * s + 1][row]), "challenge %d, lookup row %d, slot %d", c, row, s)
                            for s in range(LOOKUP_SLOTS)]                            # lookup.rs:49-56
                for slot in range(num_partial):
                    prev = polys[slot][row] if slot else polys[num_partial][row + 1]
                    polys[slot + 1][row] = (prev - sum(inverses[slot * lu_degree:min((slot + 1) * lu_degree, LOOKUP_SLOTS)])) % P
        out += polys
    return out


# ------------------------------------------------------------------------------- openings, batch reduction, division, fold
def _ext(z):
    return (int(z[0]) % P, int(z[1]) % P)


def eval_ext(coeffs, z):
    """PolynomialCoeffs::to_extension().eval(z) (proof.rs:306-344 eval_commitment): Horner in F_p^2 over base-field coefficients"""
    z, acc = _ext(z), (0, 0)
    for c in reversed([int(v) for v in coeffs]):
        acc = _ext_mul(acc, z)
        acc = ((acc[0] + c) % P, acc[1])
    return acc


def reduce_polys_base(polys, alpha, n=None):
    """ReducingFactor::reduce_polys_base (reducing.rs:83-95): sum_j alpha^j polys[j] -> n extension coefficients.  A polynomial given
    as None is the zero polynomial: it takes its power of alpha and adds nothing."""
    alpha, power = _ext(alpha), (1, 0)
    acc = [(0, 0)] * (len(next(p for p in polys if p is not None)) if n is None else n)
    for poly in polys:
        if poly is not None:
            acc = [((a + power[0] * c) % P, (b + power[1] * c) % P) for (a, b), c in zip(acc, poly)]
        power = _ext_mul(power, alpha)
    return acc


def divide_by_linear(coeffs, z):
    """PolynomialCoeffs::divide_by_linear (division.rs:75-88): (p(X) - p(z)) / (X - z), one coefficient shorter than p"""
    z, acc, bs = _ext(z), (0, 0), []
    for c in reversed(coeffs):
        acc = _ext_mul(acc, z)
        acc = ((acc[0] + c[0]) % P, (acc[1] + c[1]) % P)
        bs.append(acc)
    bs.pop()
    return bs[::-1]


def opened_polys(groups):
    """(the polynomials opened at zeta, those opened at g zeta) of the four oracles constants || sigmas, wires, Z || partial products
    (|| lookup polynomials), quotient chunks, each [columns][n] coefficients: the order of glfri::PlonkInstance in fri_instance.hpp (FriOpenings,
    proof.rs:346-380; circuit_data.rs:564-597), the lookup polynomials last in both batches"""
    cs, wires, zs, quotient = (list(grp) for grp in groups)
    return cs + wires + zs[:20] + quotient + zs[20:], zs[:2] + zs[20:]


def combine_and_divide(groups, zeta, g, alpha):
    """-> the n extension coefficients of  alpha^nnext (F0 - F0(zeta)) / (X - zeta) + (F1 - F1(g zeta)) / (X - g zeta)  (prove_openings,
    oracle.rs:183-197: per batch reduce_polys_base, divide_by_linear, the zero pushed back on, shift_poly of what came before).  `groups`:
    the four oracles' coefficient columns, a column given as None being the zero polynomial."""
    groups = [[None if col is None else _ints([col])[0] for col in grp] for grp in groups]
    zeta, alpha = _ext(zeta), _ext(alpha)
    n = len(next(col for col in groups[0] if col is not None))
    final = [(0, 0)] * n
    for polys, point in zip(opened_polys(groups), (zeta, (zeta[0] * g % P, zeta[1] * g % P))):
        quotient = divide_by_linear(reduce_polys_base(polys, alpha), point) + [(0, 0)]     # reduce_polys_base: count = len(polys)
        shift = (1, 0)
        for _ in range(len(polys)):                                 # shift_poly(final_poly): final *= alpha^count, count = 0
            shift = _ext_mul(shift, alpha)
        final = [((f[0] + q[0]) % P, (f[1] + q[1]) % P) for f, q in zip((_ext_mul(f, shift) for f in final), quotient)]
    return final


def fold(coeffs, arity, beta):
    """one commit-phase reduction (fri/prover.rs:94-103): reduce_with_powers (plonk_common.rs:116-128) of every chunk of `arity`
    coefficients by beta"""
    beta, out = _ext(beta), []
    for k in range(0, len(coeffs), arity):
        acc = (0, 0)
        for c in reversed(coeffs[k:k + arity]):
            acc = _ext_mul(acc, beta)
            acc = ((acc[0] + int(c[0])) % P, (acc[1] + int(c[1])) % P)
        out.append(acc)
    return out
