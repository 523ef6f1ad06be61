"""Fewer launches per proof, the same bytes: k_gather_pieces (the whole query phase in one table-driven gather launch) and gl_fri_combine on
the one-pass opening kernels (k_fri_combine_points<2>, k_div_points_*).  The m = 8 proof through gl_prove and through the phase API is the
oracle's byte for byte; gl_fri_query with 1 and with 84 indices is held against the oracle's bytes where the proof opened the same index,
and everywhere against the batches' own leaves and paths (gl_batch_get_leaf, gl_batch_prove: other kernels) and against the caps."""
import numpy as np
import pytest

from oracle_lib import P, rand_field
from transcript import LibraryChallenger, drive_phase_api

U64 = np.uint64


def split_query(d, batches, blob, nq):
    """gl_fri_query's bytes -> per query [(leaf words, siblings [k][4]), ...]: the four initial trees, then one per FRI round"""
    lgN = d.degree_bits + d.rate_bits
    shapes = [(b.ncols + b.salt, lgN - d.cap_height) for b in batches]
    lg = lgN
    for r in range(d.num_fri_rounds):
        lg -= d.fri_arity_bits[r]
        shapes.append((2 << d.fri_arity_bits[r], lg - d.cap_height))
    per_query = sum(8 * w + 1 + 32 * k for w, k in shapes)
    assert len(blob) == nq * per_query
    out = []
    for q in range(nq):
        pos, trees = q * per_query, []
        for w, k in shapes:
            leaf = np.frombuffer(blob, dtype="<u8", count=w, offset=pos).astype(U64)
            assert blob[pos + 8 * w] == k, "path length byte"
            sib = np.frombuffer(blob, dtype="<u8", count=4 * k, offset=pos + 8 * w + 1).astype(U64).reshape(k, 4)
            trees.append((leaf, sib))
            pos += 8 * w + 1 + 32 * k
        out.append(trees)
    return out, per_query


@pytest.mark.gpu
def test_m8_proof_and_query_blobs_of_1_and_84_queries(gpu, orc):
    p, ctx = gpu
    m = 8
    hc = p.MatmulCircuit(m)
    a, b = rand_field(4700, m * m) % (2**32 - 1), rand_field(4701, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=m)
    cd = hc.build()
    d = cd.desc
    want = orc.circuit(m, threads=8).witness(a, b, filler_seed=m).prove(threads=8).to_bytes()
    # gl_prove: one gather launch, the openings combined by the one-pass kernels
    assert cd.prove(wires, pis).to_bytes() == want
    # the phase API (gl_fri_combine ... gl_fri_query) assembles the same bytes: its query blob of the proof's own indices is the oracle's
    r = drive_phase_api(p, ctx, orc, cd, LibraryChallenger(p), wires, pis)
    assert r.bytes == want
    nq0, N = d.num_query_rounds, 1 << (d.degree_bits + d.rate_bits)
    _, per_query = split_query(d, r.batches, r.query_blob, nq0)
    chunk = {x: r.query_blob[q * per_query:(q + 1) * per_query] for q, x in enumerate(r.x_index)}
    # one query: each of the proof's, alone
    for x in (r.x_index[0], r.x_index[-1]):
        assert r.fri.query([x]) == chunk[x]
    for x in (0, N - 1):
        check_queries(orc, d, r, [x], r.fri.query([x]), chunk)
    # 84 queries (gl_fri_query takes 1..256): the proof's in reverse, both ends, and random rows; a query's bytes depend on its index alone
    xs = list(reversed(r.x_index)) + [0, N - 1, 1, N - 2]
    xs += np.random.default_rng(4702).integers(0, N, 84 - len(xs)).tolist()
    assert len(xs) == 84
    check_queries(orc, d, r, xs, r.fri.query(xs), chunk)
    with pytest.raises(p.Plonky2Mi355xError):
        r.fri.query([N])


def check_queries(orc, d, r, xs, blob, chunk):
    """Query q of `blob` is the oracle's bytes where the proof opened the same index; everywhere the initial leaves and paths are the
    batches' own (gl_batch_get_leaf, gl_batch_prove: other kernels) and every leaf, FRI rounds included, verifies against its cap
    (caps that the proof's bytes hold equal to the oracle's)."""
    queries, per_query = split_query(d, r.batches, blob, len(xs))
    for q, x in enumerate(xs):
        if x in chunk:
            assert blob[q * per_query:(q + 1) * per_query] == chunk[x], "query %d (index %d)" % (q, x)
        for o, bt in enumerate(r.batches):
            leaf, sib = queries[q][o]
            assert (leaf == bt.get_leaf(x)).all() and (sib == bt.prove(x)).all(), "query %d (index %d), initial tree %d" % (q, x, o)
            assert orc.merkle_verify(leaf, x, bt.cap, sib)
        xi = x
        for k in range(d.num_fri_rounds):
            xi >>= d.fri_arity_bits[k]
            leaf, sib = queries[q][len(r.batches) + k]
            assert (leaf < U64(P)).all()
            assert orc.merkle_verify(leaf, xi, r.fri_caps[k], sib), "query %d (index %d), FRI round %d" % (q, x, k)
