"""Mutants of a circuit proof's bytes, built with the proof parser, that the verifier tests share (no tests here): the query matrix
(d) - (h), the host-stage mutants (a) - (c), (i) - (m)."""
import numpy as np

from oracle_lib import P
from proof_parser import ParsedProof, hash_bytes, leaf_lens, opening_columns, proof_bytes

U64 = np.uint64


def _bump(a, i):
    a[i] = U64((int(a[i]) + 1) % P)


def _emit(d, pp):
    return proof_bytes(d, pp.caps, pp.openings, pp.fri_caps, pp.queries, pp.final_poly, pp.pow_witness, pp.public_inputs)


def _query_mutants(d, by, x_index, q):
    """(d) - (h) at query q: (name, bytes)"""
    out = []

    def mutant(name, change):
        pp = ParsedProof(d, by)
        change(pp.queries[q])
        out.append(("%s q%d" % (name, q), _emit(d, pp)))

    def sibling(h):                                      # a hash word: an element under Poseidon, eight raw bytes under Keccak
        if d.hasher:
            h[0] ^= U64(1)
        else:
            _bump(h, 2)

    for o in range(4):
        mutant("d: initial leaf of tree %d" % o, lambda qr, o=o: _bump(qr[0][o][0], 1))
        if d.zero_knowledge and o:
            mutant("d: salt of tree %d" % o, lambda qr, o=o: _bump(qr[0][o][0], len(qr[0][o][0]) - 1))
    mutant("e: initial sibling, first level", lambda qr: sibling(qr[0][1][1][0]))
    mutant("e: initial sibling, last level", lambda qr: sibling(qr[0][2][1][-1]))
    x = x_index[q]
    for r in range(d.num_fri_rounds):
        ab = d.fri_arity_bits[r]
        within = x & ((1 << ab) - 1)
        mutant("f: step leaf at x & 15, round %d" % r, lambda qr, r=r, w=within: _bump(qr[1][r][0], 2 * w))
        mutant("g: another step leaf entry, round %d" % r, lambda qr, r=r, w=within: _bump(qr[1][r][0], 2 * ((w + 1) % (1 << ab)) + 1))
        assert len(ParsedProof(d, by).queries[q][1][r][1]) >= 1
        mutant("h: step sibling, round %d" % r, lambda qr, r=r: sibling(qr[1][r][1][0]))
        x >>= ab
    return out


def _host_stage_mutants(d, by):
    """(a), (b), (c), (i) - (m): (name, bytes)"""
    out = []

    def mutant(name, change):
        pp = ParsedProof(d, by)
        change(pp)
        out.append((name, _emit(d, pp)))

    mutant("a: opening word", lambda pp: _bump(pp.openings["wires"], 3))

    def pow_witness(pp):
        pp.pow_witness = (pp.pow_witness + 1) % P
    mutant("b: proof-of-work witness", pow_witness)
    if d.num_public_inputs:
        mutant("c: public input", lambda pp: _bump(pp.public_inputs, 0))
    mutant("i: final polynomial coefficient", lambda pp: _bump(pp.final_poly, 1))
    out.append(("j: truncated", by[: len(by) // 2]))
    out.append(("k: trailing byte", by + b"\0"))
    ncap, hb = 1 << d.cap_height, hash_bytes(d)
    at = 3 * ncap * hb + 16 * sum(k for _, k in opening_columns(d)) + d.num_fri_rounds * ncap * hb + 8 * leaf_lens(d)[0]
    assert by[at] == d.degree_bits + d.rate_bits - d.cap_height      # the length byte of the first initial path
    out.append(("l: path length off by one", by[:at] + bytes([by[at] + 1]) + by[at + 1:]))

    bad = _non_canonical_leaf_word(d, by)
    if bad is not None:
        out.append(("m: w + p for a leaf word w", bad))
    return out


def _non_canonical_leaf_word(d, by):
    """(m): the first leaf word w < 2^32 - 1 of the proof replaced by w + p, which still fits 64 bits.  The values of a low-degree
    extension are uniform, so such a word exists only where a column is the zero polynomial (the m = 2 circuit has one, the m = 8 and
    m = 20 circuits have none): None then."""
    pp = ParsedProof(d, by)
    hit = next(((leaf, i) for init, _ in pp.queries for leaf, _ in init for i in range(len(leaf)) if int(leaf[i]) < 2**32 - 1), None)
    if hit is None:
        return None
    hit[0][hit[1]] = U64(int(hit[0][hit[1]]) + P)
    return _emit(d, pp)
