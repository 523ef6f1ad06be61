"""The Poseidon MDS layer on the i8 matrix cores (poseidon.cuh psd_mds_mfma) against the vector-ALU layer and the textbook
permutation.

CPU: the generator's MFMA tables (A operand coefficients, bias-corrected constants) reproduce the permutation in Python,
operand by operand, and the product's generated include holds exactly those tables.
GPU: one build holds both layers (gl_poseidon_permute_raw takes the layer), so they are compared on the RAW u64 words the
permutation leaves, not only on canonical values -- the MFMA layer's accumulators are the VALU layer's, bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
P = 0xFFFFFFFF00000001
LAYER_VALU, LAYER_MFMA = 0, 1


def _perm_with_mfma_layer(state, rc, G, F):
    """The GPU's round structure (grouped partial rounds) with every MDS layer of the full rounds and of the lone partial round
    computed as the MFMA layer does (gen_poseidon_constants.mds_mfma), on u64 representatives."""
    import gen_poseidon_constants as g
    s = [(x + c) % P for x, c in zip(state, rc[0])]
    r = 0
    for _ in range(g.HALF_FULL):
        _, s = g.mds_mfma([g.sbox(a) for a in s], F["A"], F["K"], r + 1); r += 1
    dot = lambda row, v: sum(a * b for a, b in zip(row, v)) % P
    for gi in range(g.N_GROUPS):
        k1, k2, K3 = G["K"][gi][0], G["K"][gi][1], G["K"][gi][2:]
        a0 = s[0]; d0 = (g.sbox(a0) - a0) % P
        a1 = (dot(G["R1"], s) + d0 * G["V0"][0] + k1) % P; d1 = (g.sbox(a1) - a1) % P
        a2 = (dot(G["R2"], s) + d0 * G["V1"][0] + d1 * G["V0"][0] + k2) % P; d2 = (g.sbox(a2) - a2) % P
        s = [(dot(G["M3"][l], s) + d0 * G["V2"][l] + d1 * G["V1"][l] + d2 * G["V0"][l] + K3[l]) % P for l in range(g.W)]
        r += g.GROUP
    while r < g.HALF_FULL + g.N_PARTIAL:
        s[0] = g.sbox(s[0])
        _, s = g.mds_mfma(s, F["A"], F["K"], r + 1); r += 1
    for _ in range(g.HALF_FULL):
        _, s = g.mds_mfma([g.sbox(a) for a in s], F["A"], F["K"], r + 1); r += 1      # r + 1 = 30 on the last: no constants
    return s


def test_mfma_tables_reproduce_the_textbook_permutation():
    import gen_poseidon_constants as g
    rc = g.load_round_constants()
    T = g.derive(rc)
    G = g.derive_groups(rc, T["M"])
    F = g.derive_mfma(rc)
    rng = np.random.default_rng(5)
    states = [[0] * 12, [P - 1] * 12, [2**64 - 1] * 12, [0x7F7F7F7F7F7F7F7F] * 12, [0x8080808080808080] * 12]
    states += [[int(x) for x in rng.integers(0, 2**64, 12, dtype=np.uint64)] for _ in range(6)]
    for st in states:
        assert _perm_with_mfma_layer(st, rc, G, F) == g.perm_naive(st, rc, T["M"])
    for inp, out in g.KATS:
        assert _perm_with_mfma_layer(inp, rc, G, F) == out


def test_mfma_layer_accumulators_equal_the_valu_ones_on_edge_bytes():
    # every byte 0x00 / 0x7f / 0x80 / 0xff (the i8 bias boundary) in every half, with and without round constants
    import gen_poseidon_constants as g
    rc = g.load_round_constants()
    F = g.derive_mfma(rc)
    M = g.mds_matrix()
    rng = np.random.default_rng(6)
    byte_vals = [0x00, 0x7F, 0x80, 0xFF]
    for _ in range(40):
        st = [int.from_bytes(bytes(int(b) for b in rng.choice(byte_vals, 8)), "little") for _ in range(12)]
        for n in (1, 5, 29, 30):
            acc, out = g.mds_mfma(st, F["A"], F["K"], n)
            cst = rc[n] if n < 30 else [0] * 12
            lo, hi = [x & 0xFFFFFFFF for x in st], [x >> 32 for x in st]
            assert acc == [(cst[i] % 2**32 + sum(M[i][j] * lo[j] for j in range(12)), (cst[i] >> 32) + sum(M[i][j] * hi[j] for j in range(12)))
                           for i in range(12)]
            assert out == [(sum(M[i][j] * st[j] for j in range(12)) + cst[i]) % P for i in range(12)]


def test_product_include_holds_the_generated_mfma_tables():
    import re
    import gen_poseidon_constants as g
    F = g.derive_mfma(g.load_round_constants())
    text = open(os.path.join(ROOT, "plonky2_demo_amd", "csrc", "poseidon_constants.inc")).read()
    tables = {}
    for m in re.finditer(r"POSEIDON_TABLE(?:32)?\((\w+), (\d+)\) = \{(.*?)\};", text, re.S):
        vals = [int(x.rstrip("uUL"), 0) for x in re.findall(r"0x[0-9a-fA-F]+|\b\d+u?\b", m.group(3))]
        assert len(vals) == int(m.group(2))
        tables[m.group(1)] = vals
    assert tables["POSEIDON_MDS_I8A"] == F["A"]
    assert tables["POSEIDON_MDS_K"] == F["K"]
    assert max(max((w >> (8 * b)) & 0xFF for b in range(4)) for w in F["A"]) < 128     # i8 operands


# ------------------------------------------------------------------------------------------------------------------ GPU
def _permute_raw(ctx, states, layer):
    from plonky2_demo_amd._lib import check, lib
    s = np.ascontiguousarray(states, dtype=np.uint64)
    d = ctx.alloc(s.nbytes).upload(s)
    check(lib.gl_poseidon_permute_raw(ctx.handle, ctypes.c_void_p(d.ptr), s.shape[0], layer))
    out = d.download(s.shape)
    d.free()
    return out


def _edge_states(seed, count):
    rng = np.random.default_rng(seed)
    full = lambda v: np.full(12, v, dtype=np.uint64)
    states = [full(0), full(P - 1), full(P), full(2**64 - 1), full(0x7F7F7F7F7F7F7F7F), full(0x8080808080808080),
              full(0xFFFFFFFFFFFFFFFF), full(0x80808080FFFFFFFF), full(0x7F7F7F7F80808080)]
    byte_vals = np.array([0x00, 0x7F, 0x80, 0xFF], dtype=np.uint8)
    for _ in range(200):                                        # every word from the bytes 0x00 / 0x7f / 0x80 / 0xff
        states.append(rng.choice(byte_vals, 96).view(np.uint64).copy())
    for _ in range(200):                                        # non-canonical words (>= p)
        states.append(rng.integers(P, 2**64, 12, dtype=np.uint64, endpoint=False))
    states = np.stack(states)
    rnd = rng.integers(0, 2**64, (count - len(states), 12), dtype=np.uint64)
    return np.concatenate([states, rnd])


@pytest.mark.gpu
@pytest.mark.parametrize("count", [37, 64 * 40 + 5, 1 << 14])
def test_mfma_and_valu_layers_leave_identical_raw_words(gpu, orc, count):
    # launches that are not a multiple of 64 leave a partial last wave: its lanes past the end must not disturb the others
    p, ctx = gpu
    states = _edge_states(count, max(count, 1000))[:count]
    valu = _permute_raw(ctx, states, LAYER_VALU)
    mfma = _permute_raw(ctx, states, LAYER_MFMA)
    assert (valu == mfma).all(), "MFMA layer differs from the VALU layer in %d words" % int((valu != mfma).sum())
    canon = np.where(mfma >= np.uint64(P), mfma - np.uint64(P), mfma)
    assert (canon == orc.poseidon(states)).all()


@pytest.mark.gpu
def test_mfma_layer_known_answers(gpu, golden):
    p, ctx = gpu
    for kat in golden["poseidon_kats"]:
        got = _permute_raw(ctx, np.array([kat["input"]], dtype=np.uint64), LAYER_MFMA)[0]
        assert [int(x) % P for x in got] == kat["output"]
