"""The Python-integer model of the permutation, lookup, opening and FRI-reduction phases (tests/prover_phase_model.py) on its own
evidence, before it judges a kernel (tests/test_prover_phases.py).  CPU only.

Against the oracle's prover, on its proofs of the m = 1 and m = 3 matmul circuits and of the circuit with every oracle gate (kind 15,
two lookup tables): Z, the partial products and the lookup polynomials; the openings in the proof bytes; the polynomial that goes into
FRI; the final polynomial after the proof's own folds.  Only the inputs, the transforms (pinned elsewhere) and the parser of the bytes
come from outside the model.  On edge operands, which no proof carries, the oracle's stand-alone reduce_polys_base and divide_by_linear
against the model's."""
import numpy as np
import pytest

import prover_phase_model as pm
from proof_parser import ParsedProof
from test_quotient_model import EDGES
from test_vanishing_model import _kind, _matmul, oracle_inputs

P = pm.P
# opening points and reduction challenges: base-field elements (0 among them), elements with a zero real part, edge words in both
# halves, a seeded random one and a non-canonical one (read mod p)
ZETAS = [(0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1), (P - 1, P - 1), (2**32, 2**32 - 1),
         tuple(int(v) for v in np.random.Generator(np.random.PCG64(2024)).integers(0, P, size=2, dtype=np.uint64)), (P + 3, 2**64 - 1)]

CASES = {"matmul m = 1": lambda orc: _matmul(orc, 1), "matmul m = 3": lambda orc: _matmul(orc, 3),
         "kind 15: two lookup tables": lambda orc: _kind(orc, 15, 1, [0, 0])}
# the three circuits above are too short for a reduction round: the fold is pinned on m = 8 (n = 2^7, one round of arity 16)
FOLDING = {"matmul m = 8": lambda orc: _matmul(orc, 8)}
_proved = {}


def proved(orc, name):
    """one oracle proof per circuit for the whole module: (desc, constants || sigmas, wires, zs, betas, gammas, deltas, proof, its parsed bytes)"""
    if name not in _proved:
        oc, w = {**CASES, **FOLDING}[name](orc)
        d, (cs, wires, zs), _, betas, gammas, _, deltas, op = oracle_inputs(orc, oc, w)
        _proved[name] = (d, cs, wires, zs, betas, gammas, deltas, op, ParsedProof(d, op.to_bytes()))
    return _proved[name]


def lookup_rows(d):
    return [(d.last_lu_row[t], d.last_lut_row[t], d.first_lut_row[t]) for t in range(d.num_luts)]


def pairs(words):
    return [(int(words[2 * k]), int(words[2 * k + 1])) for k in range(len(words) // 2)]


@pytest.mark.parametrize("name", list(CASES))
def test_partial_products_and_lookup_polys_are_the_oracles(orc, name):
    d, cs, wires, zs, betas, gammas, deltas, op, _ = proved(orc, name)
    got = pm.partial_products(wires, cs[d.num_constants:], [int(d.k_is[j]) for j in range(80)], betas, gammas, d.degree_bits)
    if d.num_lookup_polys:
        assert d.num_luts == 2 and d.num_lookup_polys == pm.NUM_LOOKUP_POLYS
        got += pm.lookup_polys(wires, lookup_rows(d), deltas)
    assert len(got) == len(zs) and (np.array(got, dtype=np.uint64) == zs).all()


@pytest.mark.parametrize("name", list(CASES))
def test_eval_ext_reproduces_the_openings_in_the_proof_bytes(orc, name):
    d, cs, wires, zs, _, _, _, op, pp = proved(orc, name)
    zeta = op.challenges()["zeta"]
    g = pm.primitive_root(d.degree_bits)
    gzeta = [zeta[0] * g % P, zeta[1] * g % P]
    cs_c, wires_c, zs_c, q_c = orc.ifft(cs), orc.ifft(wires), orc.ifft(zs), op.quotient_chunks()
    nc, o = d.num_constants, pp.openings
    for what, polys, point in (("constants", cs_c[:nc], zeta), ("sigmas", cs_c[nc:], zeta), ("wires", wires_c, zeta), ("zs", zs_c[:2], zeta),
                               ("zs_next", zs_c[:2], gzeta), ("lookups", zs_c[20:], zeta), ("lookups_next", zs_c[20:], gzeta),
                               ("pp", zs_c[2:20], zeta), ("quotient", q_c, zeta)):
        assert [pm.eval_ext(c, point) for c in polys] == pairs(o[what]), what


@pytest.mark.parametrize("name", list(CASES) + list(FOLDING))
def test_combine_and_divide_is_the_polynomial_the_oracle_feeds_into_fri_and_fold_gives_its_final_polynomial(orc, name):
    d, cs, wires, zs, _, _, _, op, pp = proved(orc, name)
    ch = op.challenges()
    groups = [orc.ifft(cs), orc.ifft(wires), orc.ifft(zs), op.quotient_chunks()]
    got = pm.combine_and_divide(groups, ch["zeta"], pm.primitive_root(d.degree_bits), ch["fri_alpha"])
    assert (np.array(got, dtype=np.uint64) == op.final_poly_initial()).all()
    assert len(ch["fri_betas"]) == d.num_fri_rounds and (d.num_fri_rounds >= 1) == (name in FOLDING)
    for r, beta in enumerate(ch["fri_betas"]):
        got = pm.fold(got, 1 << d.fri_arity_bits[r], beta)
    assert got == pairs(pp.final_poly)


@pytest.mark.parametrize("z", ZETAS, ids=lambda z: "%x,%x" % z)
def test_reduction_and_division_parts_agree_with_the_oracles_on_edge_operands(orc, z):
    # 5 polynomials of 64 coefficients drawn from EDGES, reduced by alpha = z and divided by X - z; the oracle takes canonical words
    rng = np.random.Generator(np.random.PCG64(64))
    polys = np.array(EDGES, dtype=np.uint64)[rng.integers(0, len(EDGES), size=(5, 64))]
    polys[0, :3], polys[1, -3:] = [0, 1, P - 1], [P - 1, 0, 0]
    canonical = [z[0] % P, z[1] % P]
    reduced = pm.reduce_polys_base([[int(v) for v in p] for p in polys], z)
    assert (np.array(reduced, dtype=np.uint64) == orc.reduce_polys_base(canonical, polys)).all()
    quotient = pm.divide_by_linear(reduced, z)
    assert len(quotient) == 63 and (np.array(quotient, dtype=np.uint64) == orc.divide_by_linear(np.array(reduced, dtype=np.uint64), canonical)).all()
    # and the defining identity: q(X) (X - z) + p(z) = p(X), coefficient by coefficient
    zc, pz = tuple(canonical), (0, 0)
    for c in reversed(reduced):
        pz = pm._ext_mul(pz, zc)
        pz = ((pz[0] + c[0]) % P, (pz[1] + c[1]) % P)
    for k in range(64):
        hi = quotient[k - 1] if k else (0, 0)
        lo = pm._ext_mul(quotient[k], zc) if k < 63 else (0, 0)
        want = tuple((hi[i] - lo[i] + (pz[i] if k == 0 else 0)) % P for i in range(2))
        assert want == reduced[k], k
