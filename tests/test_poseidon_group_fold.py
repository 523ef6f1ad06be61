"""The partial-round groups of the Poseidon permutation with d_0 folded into the state (poseidon.cuh psd_partial_group,
tools/gen_poseidon_constants.py perm_grouped_folded): word 0 is replaced by sbox(x_0) before the three linear maps, so the d_0 terms
(d_0 times column 0 of M, M^2 and M^3) disappear.

The last step of a group, M^3 s, was also built on the i8 matrix cores and measured; it lost to this form and is not in the tree
(profiles/README.md, "Partial-round groups on the matrix cores"), so the cases of that issue that test its tables have nothing to test.
CPU: the folded formulation is the grouped and the textbook permutation, and the four known answers; M^3 has 21-bit entries, as the
generator asserts; the product's include holds the derived group tables.
GPU: gl_poseidon_permute_raw leaves identical raw words with both MDS layers on states whose words ENTERING groups 0, 3 and 6 are made of
the bytes 0x00 / 0x7f / 0x80 / 0xff, words >= p and all-ones; Merkle trees, hashed rows and the proof-of-work grind run the group inside
the hash kernels, against the oracle."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_poseidon_constants as g  # noqa: E402

P = g.P
EDGE_BYTES = [0x00, 0x7F, 0x80, 0xFF]
_T = None


def tables():
    global _T
    if _T is None:
        rc = g.load_round_constants()
        M = g.mds_matrix()
        G = g.derive_groups(rc, M)
        _T = dict(rc=rc, M=M, Minv=g.mat_inv(M), G=G)
    return _T


def edge_word(rng):
    return int.from_bytes(bytes(int(b) for b in rng.choice(EDGE_BYTES, 8)), "little")


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_group_matrices_have_the_asserted_widths_and_columns():
    G = tables()["G"]
    assert max(max(r) for r in G["M3"]).bit_length() == 21 and max(G["R2"]).bit_length() == 13
    # what the fold rests on: the d_0 coefficients are column 0 of M, M^2 and M^3
    assert G["V2"] == [row[0] for row in G["M3"]] and G["V1"][0] == G["R2"][0] and G["V0"][0] == G["R1"][0] == 25
    # an accumulator of the last step stays below 2^63 (glx_acc_reduce3): K3 half + 12 M^3 terms + the d_1 and d_2 terms
    worst = 2**32 + (2**32 - 1) * (max(sum(r) for r in G["M3"]) + max(G["V1"]) + max(G["V0"]))
    assert worst < 2**63


def test_folded_groups_equal_the_grouped_and_the_textbook_permutation(golden):
    T = tables()
    rng = np.random.default_rng(76)
    states = [[0] * 12, [P - 1] * 12, list(range(12)), [2**64 - 1] * 12, [0x7F7F7F7F80808080] * 12]
    states += [[edge_word(rng) for _ in range(12)] for _ in range(8)] + [[int(x) for x in rng.integers(0, 2**64, 12, dtype=np.uint64)] for _ in range(8)]
    for st in states:
        want = g.perm_grouped(st, T["rc"], T["M"], T["G"])
        assert g.perm_grouped_folded(st, T["rc"], T["M"], T["G"]) == want == g.perm_naive(st, T["rc"], T["M"])
    assert len(golden["poseidon_kats"]) == 4
    for kat in golden["poseidon_kats"]:
        assert g.perm_grouped_folded(kat["input"], T["rc"], T["M"], T["G"]) == kat["output"]


def test_product_include_holds_the_generated_group_tables():
    T = tables()
    text = open(os.path.join(ROOT, "plonky2_demo_amd", "csrc", "poseidon_constants.inc")).read()
    found = {}
    for m in re.finditer(r"POSEIDON_TABLE(?:32)?\((\w+), (\d+)\) = \{(.*?)\};", text, re.S):
        vals = [int(x.rstrip("uUL"), 0) for x in re.findall(r"0x[0-9a-fA-F]+|\b\d+u?\b", m.group(3))]
        assert len(vals) == int(m.group(2))
        found[m.group(1)] = vals
    G = T["G"]
    assert found["POSEIDON_G3_M3"] == [x for row in G["M3"] for x in row]
    assert found["POSEIDON_G3_R2"] == G["R2"] and found["POSEIDON_G3_V1"] == G["V1"] and found["POSEIDON_G3_V2"] == G["V2"]
    assert found["POSEIDON_G3_K"] == [x for row in G["K"] for x in row] and len(found["POSEIDON_G3_K"]) == 7 * 14


# ----------------------------------------------------------------------------------------------------------------- GPU
def _group_entry_states(count, seed):
    """`count` permutation inputs.  Lane k of every wave of 64: k % 4 == 0..2 -> the state ENTERING group 0 / 3 / 6 (right after the
    constants of round 4 / 13 / 22) is made of edge bytes (as field values); k % 4 == 3 -> random.  Then words >= p and all-ones."""
    T = tables()
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2**64, (count, 12), dtype=np.uint64)
    entering = {}
    for k in range(count):
        if k % 4 < 3:
            round_ = 4 + 9 * (k % 4)
            target = [edge_word(rng) % P for _ in range(12)]
            out[k] = g.perm_naive_to_input(target, round_, T["rc"], T["Minv"])
            entering[k] = (round_, target)
    for k, fill in ((count - 1, 2**64 - 1), (count - 2, P), (count - 3, P + 0x7F7F7F7F)):
        out[k] = np.uint64(fill)
        entering.pop(k, None)
    out[count - 4] = rng.integers(P, 2**64, 12, dtype=np.uint64, endpoint=False)
    entering.pop(count - 4, None)
    return out, entering


_STATES = {}


def group_entry_states(count):
    if count not in _STATES:
        _STATES[count] = _group_entry_states(count, 800 + count)
    return _STATES[count]


def test_crafted_states_enter_their_group_as_edge_bytes():
    T = tables()
    st, entering = group_entry_states(37)
    assert {r for r, _ in entering.values()} == {4, 13, 22}
    for k, (round_, target) in entering.items():
        trace, _ = g.sbox_inputs([int(x) for x in st[k]], T["rc"], T["M"])
        assert trace[round_] == target


@pytest.mark.gpu
@pytest.mark.parametrize("count", [37, 64 * 2 + 5])
def test_both_layers_leave_identical_raw_words_on_group_edge_states(gpu, orc, count):
    from test_poseidon_variants import LAYER_MFMA, LAYER_VALU, _permute_raw
    p, ctx = gpu
    st, _ = group_entry_states(count)
    valu = _permute_raw(ctx, st, LAYER_VALU)
    mfma = _permute_raw(ctx, st, LAYER_MFMA)
    assert (valu == mfma).all(), "the layers differ at states %s" % np.argwhere((valu != mfma).any(axis=1)).ravel()[:8]
    want = orc.poseidon(st)
    assert (valu % np.uint64(P) == want).all()
    assert (p.poseidon(st, ctx=ctx) == want).all()


def _bitrev(n):
    lg = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % lg)[::-1], 2) if lg else 0 for i in range(n)])


# 2^7 leaves: below the cooperative threshold by default; 2^14: k_merkle_leaves<WPE>, one leaf per lane, the sponge loop over the group
@pytest.mark.gpu
@pytest.mark.parametrize("width", [135, 20])
@pytest.mark.parametrize("lg", [7, 14])
def test_merkle_tree_matches_the_oracle(gpu, orc, lg, width):
    p, ctx = gpu
    n = 1 << lg
    rng = np.random.default_rng(900 + lg + width)
    leaves = rng.integers(0, P, (n, width), dtype=np.uint64)
    leaves[1] = rng.choice(np.array(EDGE_BYTES, dtype=np.uint8), 8 * width).view(np.uint64) % np.uint64(P)
    gt = p.MerkleTree(leaves, 1, ctx=ctx)
    ot = orc.merkle(leaves, 1)
    assert (gt.cap == ot.cap).all()
    for j in (1, n - 3):
        assert (gt.prove(j) == ot.prove(j)).all()
    for j in (0, 1):
        assert (p.hash_or_noop(leaves[j], ctx=ctx) == orc.hash_or_noop(leaves[j])).all()          # k_hash_rows


@pytest.mark.gpu
@pytest.mark.parametrize("buffer_len", [0, 5])
def test_pow_grind_at_eight_bits_finds_the_oracles_witness(gpu, orc, buffer_len):
    p, ctx = gpu
    bits = 8
    state = np.random.default_rng(950 + buffer_len).integers(0, P, 12, dtype=np.uint64)
    witness = p.pow_grind(state, state[:buffer_len], bits, ctx=ctx)
    want = None
    for base in range(0, 1 << 16, 1 << 12):                                   # the smallest w whose response has the leading zeros
        cand = np.arange(base, base + (1 << 12), dtype=np.uint64)
        states = np.tile(state, (len(cand), 1))
        states[:, buffer_len] = cand
        ok = np.flatnonzero(orc.poseidon(states)[:, 7] >> np.uint64(64 - bits) == 0)
        if len(ok):
            want = int(cand[ok[0]])
            break
    assert want is not None and witness == want
