"""The permutation's partial rounds in groups of four linear maps (poseidon.cuh psd_partial_group4, tools/gen_poseidon_constants.py
derive_groups4 / perm_grouped4): the 23 maps behind the S-box layer of full round 3 run as 4 + 4 + 4 + 4 + 4 + 3, six dense maps.

M^4 has 29-bit entries and row sums up to 1.04 2^32, so a 64-bit accumulator of a four-map group's last step can wrap, once.  Column 0
of M^4 is added last and the carry-out of that multiply-add goes to glx_acc_reduce3w (2^64 = 2^32 - 1 for the lo accumulator,
2^96 = -1 for the hi one).  The three-map group's entries have 21 bits: 12 terms of 53 bits cannot reach 2^64, so its all-maximal
state is run and its flags are asserted CLEAR.

Wrap cases, built backwards through the rounds (perm_naive_to_input, seventh roots for the words that enter the maps S-boxed):
  max  -- the folded state entering the dense step is twelve times 0xFFFFFFFE_FFFFFFFF (p - 2): lo and hi accumulators wrap;
  tip  -- every lo (or hi) half is h = ceil(2^64 (1 + 2^-8) / rowsum_0(M^4)), the other halves are small: only row 0, the largest row
          sum, passes 2^64, by about 2^56 (the d_i terms stay below 2^54), and only with its last term;
  near -- the tip case with half 0 lowered by the smallest power of two that takes the sum below 2^64 again: no wrap.
The model works on canonical words.  The crafted folded states are canonical words at or above 2^32 - 1, which have one 64-bit
representative, so the halves the device multiplies are the model's.

CPU: the model equals the folded and the textbook permutation and the known answers; widths; the include holds the generated tables;
the wrap flags are where the cases want them.
GPU: raw words of both MDS layers are identical and canonical values equal the oracle's on 37 and 133 states made of the cases, edge
bytes entering each group, words >= p and all-ones; Merkle trees, hashed rows and the proof-of-work grind against the oracle."""
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
HEAD, MIDDLE, TAIL = 0, 2, 5                 # the groups the cases aim at: maps 0-3, 8-11 and the three-map group 20-22
_T = None
_CASES = None
_STATES = {}


def tables():
    global _T
    if _T is None:
        rc = g.load_round_constants()
        M = g.mds_matrix()
        _T = dict(rc=rc, M=M, Minv=g.mat_inv(M), G=g.derive_groups(rc, M), G4=g.derive_groups4(rc, M))
    return _T


def edge_word(rng):
    return int.from_bytes(bytes(int(b) for b in rng.choice(EDGE_BYTES, 8)), "little")


def input_for_folded_state(n, folded):
    """The permutation input whose state entering the maps of group n (word 0 S-boxed; the head group: every word) is `folded`."""
    T = tables()
    if n == 0:
        return g.perm_naive_to_input([g.sbox_inv(x) for x in folded], g.HALF_FULL - 1, T["rc"], T["Minv"])
    round_ = T["G4"]["first_map"][n] + 3       # the S-box in front of map m is that of round m + 3
    return g.perm_naive_to_input([g.sbox_inv(folded[0])] + list(folded[1:]), round_, T["rc"], T["Minv"])


def group_trace(state, n):
    T = tables()
    trace = []
    out = g.perm_grouped4(state, T["rc"], T["M"], T["G4"], trace)
    return trace[n], out


def wrapped(step):
    """{(word, 'lo' | 'hi')} of the accumulators of a group's last step that wrapped"""
    _, _, _, acc = step
    return {(l, h) for l, (_, _, wl, wh) in enumerate(acc) for h, w in (("lo", wl), ("hi", wh)) if w}


def _tip_state(half, rng, h):
    small = lambda: int(rng.integers(0, 1 << 16))
    return [(h if half == "lo" else small()) | ((h if half == "hi" else small()) << 32) for _ in range(12)]


def cases():
    """[(name, group, input state, expected set of wrapped accumulators or None for 'at least one lo and one hi')]"""
    global _CASES
    if _CASES is not None:
        return _CASES
    T = tables()
    rng = np.random.default_rng(404)
    h = -(-(2**64 + 2**56) * 1 // sum(T["G4"]["M4"][0]))
    out = []
    for n in (HEAD, MIDDLE, TAIL):
        out.append(("max", n, input_for_folded_state(n, [0xFFFFFFFEFFFFFFFF] * 12), None if n != TAIL else set()))
        if n == TAIL:
            continue
        for half in ("lo", "hi"):
            folded = _tip_state(half, rng, h)
            st = input_for_folded_state(n, folded)
            out.append(("tip " + half, n, st, {(0, half)}))
            shift = 0 if half == "lo" else 32
            for k in range(32):
                near = [folded[0] - (1 << (k + shift))] + folded[1:]
                st_near = input_for_folded_state(n, near)
                if not wrapped(group_trace(st_near, n)[0]):
                    break
            out.append(("near " + half, n, st_near, set()))
    _CASES = out
    return out


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_groups_of_four_equal_the_folded_and_the_textbook_permutation(golden):
    T = tables()
    rng = np.random.default_rng(77)
    states = [[0] * 12, [P - 1] * 12, [2**64 - 1] * 12]
    states += [[edge_word(rng) for _ in range(12)] for _ in range(8)] + [[int(x) for x in rng.integers(0, 2**64, 12, dtype=np.uint64)] for _ in range(8)]
    for st in states:
        want = g.perm_naive(st, T["rc"], T["M"])
        assert g.perm_grouped4(st, T["rc"], T["M"], T["G4"]) == want
        assert g.perm_grouped_folded(st, T["rc"], T["M"], T["G"]) == want
    assert len(golden["poseidon_kats"]) == 4
    for kat in golden["poseidon_kats"]:
        assert g.perm_grouped4(kat["input"], T["rc"], T["M"], T["G4"]) == kat["output"]
        assert g.perm_grouped_folded(kat["input"], T["rc"], T["M"], T["G"]) == kat["output"] == g.perm_naive(kat["input"], T["rc"], T["M"])


def test_group_matrices_have_the_asserted_widths_and_term_order():
    G4 = tables()["G4"]
    assert G4["split"] == [4, 4, 4, 4, 4, 3] and G4["first_map"] == [0, 4, 8, 12, 16, 20]
    assert max(max(r) for r in G4["M4"]).bit_length() == 29
    assert max(max(r) for r in G4["M3"]).bit_length() == 21 and max(r[0] for r in G4["M3"]).bit_length() == 21
    H = 2**32 - 1
    for l in range(12):
        row = G4["M4"][l]
        assert row[0] == max(row)                                           # the term that goes last
        before_last = H + H * (G4["M1"][l][0] + sum(row[1:]) + G4["M3"][l][0] + G4["M2"][l][0])
        assert before_last < 2**64 <= before_last + H * row[0] < 2**65      # only the last term can carry, and only once
    # the lone accumulators (a_1, a_2, a_3) and the three-map group's last step stay below 2^63 (glx_acc_reduce, glx_acc_reduce3)
    assert H + H * (sum(G4["M3"][0]) + G4["M2"][0][0] + G4["M1"][0][0]) < 2**63
    assert H + H * (max(sum(r) for r in G4["M3"]) + max(r[0] for r in G4["M2"]) + max(r[0] for r in G4["M1"])) < 2**63
    # the G3 tables the kernels share with the three-round groups are these powers
    G = tables()["G"]
    assert G["M3"] == G4["M3"] and G["R2"] == G4["M2"][0] and G["V1"] == [r[0] for r in G4["M2"]] and G["V2"] == [r[0] for r in G4["M3"]]


def test_product_include_holds_the_generated_group4_tables():
    G4 = tables()["G4"]
    csrc = os.path.join(ROOT, "plonky2_demo_amd", "csrc")
    text = open(os.path.join(csrc, "poseidon_constants.inc")).read()
    found = {}
    for m in re.finditer(r"POSEIDON_TABLE(?:32)?\((\w+), (\d+)\) = \{(.*?)\};", text, re.S):
        vals = [int(x.rstrip("uUL"), 0) for x in re.findall(r"0x[0-9a-fA-F]+|\b\d+u?\b", m.group(3))]
        assert len(vals) == int(m.group(2))
        found[m.group(1)] = vals
    assert {k for k in found if k.startswith("POSEIDON_G4_")} == {"POSEIDON_G4_M4", "POSEIDON_G4_K"}
    assert found["POSEIDON_G4_M4"] == [x for row in G4["M4"] for x in row]
    assert found["POSEIDON_G4_K"] == [x for row in G4["K"] for x in row] and len(found["POSEIDON_G4_K"]) == 5 * 15 + 14
    assert re.search(r"^#define POSEIDON_G4_GROUPS 5\b", open(os.path.join(csrc, "poseidon_constants.h")).read(), re.M)


def test_wrap_cases_wrap_where_they_are_meant_to():
    T = tables()
    seen = set()
    for name, n, st, want in cases():
        assert all(0 <= x < P for x in st)
        step, out = group_trace(st, n)
        assert out == g.perm_naive(st, T["rc"], T["M"]), (name, n)
        got = wrapped(step)
        if name == "max":
            assert step[1] == [0xFFFFFFFEFFFFFFFF] * 12
            if want is None:
                assert any(h == "lo" for _, h in got) and any(h == "hi" for _, h in got), (name, n)
            else:
                assert got == set() and step[0] == 3            # the three-map group cannot wrap
        else:
            assert got == want, (name, n, got)
        if name.startswith("near"):
            # a neighbour of the tip case: one half of word 0 lower by a power of two, every other word of the folded state the same
            tip = next(group_trace(s, n)[0] for nm, k, s, _ in cases() if k == n and nm == "tip " + name.split()[1])
            diff = tip[1][0] - step[1][0]
            assert tip[1][1:] == step[1][1:] and diff > 0 and diff & (diff - 1) == 0
        seen.add((name.split()[0], n))
    assert seen == {("max", HEAD), ("tip", HEAD), ("near", HEAD), ("max", MIDDLE), ("tip", MIDDLE), ("near", MIDDLE), ("max", TAIL)}


# ----------------------------------------------------------------------------------------------------------------- GPU
def _crafted_states(count, seed):
    """`count` permutation inputs: the wrap cases (again at the start of the second wave of a longer launch), states whose folded state
    ENTERING each of the six groups is made of edge bytes, random ones, then words >= p and all-ones."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 2**64, (count, 12), dtype=np.uint64)
    entering = {}
    k = 0
    for start in (0, 64):
        if start + len(cases()) + 6 > count - 4:
            break
        k = start
        for _, _, st, _ in cases():
            out[k] = np.array(st, dtype=np.uint64); k += 1
        for n in range(6):
            folded = [edge_word(rng) % P for _ in range(12)]
            out[k] = np.array(input_for_folded_state(n, folded), dtype=np.uint64)
            entering[k] = (n, folded); k += 1
    for j, fill in ((count - 1, 2**64 - 1), (count - 2, P), (count - 3, P + 0x7F7F7F7F)):
        out[j] = np.uint64(fill)
    out[count - 4] = rng.integers(P, 2**64, 12, dtype=np.uint64, endpoint=False)
    return out, entering


def crafted_states(count):
    if count not in _STATES:
        _STATES[count] = _crafted_states(count, 1200 + count)
    return _STATES[count]


def test_crafted_states_hold_the_cases_and_edge_bytes_entering_every_group():
    st, entering = crafted_states(37)
    assert len(cases()) == 11 and st.shape == (37, 12) and sorted(n for n, _ in entering.values()) == list(range(6))
    for k, (n, folded) in entering.items():
        assert group_trace([int(x) for x in st[k]], n)[0][1] == folded
    st2, entering2 = crafted_states(64 * 2 + 5)
    assert len(entering2) == 12 and (st2[64:64 + 11] == st2[:11]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [37, 64 * 2 + 5])
def test_both_layers_leave_identical_raw_words_on_wrap_and_edge_states(gpu, orc, count):
    from test_poseidon_variants import LAYER_MFMA, LAYER_VALU, _permute_raw
    p, ctx = gpu
    st, _ = crafted_states(count)
    valu = _permute_raw(ctx, st, LAYER_VALU)
    mfma = _permute_raw(ctx, st, LAYER_MFMA)
    assert (valu == mfma).all(), "the layers differ at states %s" % np.argwhere((valu != mfma).any(axis=1)).ravel()[:8]
    want = orc.poseidon(st)
    bad = np.argwhere((valu % np.uint64(P) != want).any(axis=1)).ravel()
    assert len(bad) == 0, "states %s differ from the oracle (the first %d are the wrap cases %s)" % (bad[:8], len(cases()), [(c[0], c[1]) for c in cases()])
    assert (p.poseidon(st, ctx=ctx) == want).all()


def _wrap_row(width):
    words = [w for _, _, st, _ in cases() for w in st]
    return np.array([words[i % len(words)] for i in range(width)], dtype=np.uint64)


# 2^7 leaves: below the cooperative threshold by default; 2^14: k_merkle_leaves<WPE>, one leaf per lane, and k_merkle_level
@pytest.mark.gpu
@pytest.mark.parametrize("width", [135, 20])
@pytest.mark.parametrize("lg", [7, 14])
def test_merkle_tree_matches_the_oracle(gpu, orc, lg, width):
    p, ctx = gpu
    n = 1 << lg
    rng = np.random.default_rng(1300 + lg + width)
    leaves = rng.integers(0, P, (n, width), dtype=np.uint64)
    leaves[1] = _wrap_row(width)
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
    state = np.random.default_rng(1350 + buffer_len).integers(0, P, 12, dtype=np.uint64)
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
