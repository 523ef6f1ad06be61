#!/usr/bin/env python3
"""Derive the Poseidon-Goldilocks (width 12, x^7, 4+22+4 rounds) constant tables.

Inputs (data): tools/poseidon_round_constants.txt (30x12 round constants) and the
MDS definition circ/diag (reference: plonky2/src/hash/poseidon_goldilocks.rs:24-25).

Everything else -- the "fast partial round" tables the reference hard-codes at
plonky2/src/hash/poseidon_goldilocks.rs:27-215 -- is DERIVED here from first principles
(Poseidon paper, appendix B: push the partial-round constants through the linear layer
and factor the MDS matrix into one dense pre-matrix and 22 sparse matrices), then checked
against (a) naive-vs-fast permutation equality and (b) the four known-answer vectors of
plonky2/src/hash/poseidon_goldilocks.rs:449-485.

Output: a C/HIP include file with the tables, shared by oracle/ and the HIP kernels.

Usage: python tools/gen_poseidon_constants.py [out.h]
"""
import os
import sys

P = 0xFFFFFFFF00000001
W = 12
HALF_FULL = 4
N_PARTIAL = 22
N_ROUNDS = 2 * HALF_FULL + N_PARTIAL
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]

HERE = os.path.dirname(os.path.abspath(__file__))


def load_round_constants():
    rows = []
    with open(os.path.join(HERE, "poseidon_round_constants.txt")) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            rows.append([int(x, 16) for x in line.split()])
    assert len(rows) == N_ROUNDS and all(len(r) == W for r in rows)
    return rows


def mds_matrix():
    # column-vector convention: out[r] = sum_c M[r][c] * in[c]; M[r][c] = circ[(c-r) mod 12] (+diag)
    M = [[MDS_CIRC[(c - r) % W] % P for c in range(W)] for r in range(W)]
    for r in range(W):
        M[r][r] = (M[r][r] + MDS_DIAG[r]) % P
    return M


def mat_mul(A, B):
    n, k, m = len(A), len(B), len(B[0])
    return [[sum(A[i][t] * B[t][j] for t in range(k)) % P for j in range(m)] for i in range(n)]


def mat_vec(A, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in A]


def mat_inv(A):
    n = len(A)
    M = [row[:] + [1 if i == j else 0 for j in range(n)] for i, row in enumerate(A)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] % P)
        M[c], M[piv] = M[piv], M[c]
        inv = pow(M[c][c], P - 2, P)
        M[c] = [x * inv % P for x in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [(x - f * y) % P for x, y in zip(M[r], M[c])]
    return [row[n:] for row in M]


def derive(rc):
    M = mds_matrix()
    Minv = mat_inv(M)
    # --- constants: push partial-round constants backwards through M ---------------------
    # naive: x <- M * S(x + c_r); fast: y <- M * (S(y) + k_r e0), with y_0 = x_0 + first
    part = rc[HALF_FULL:HALF_FULL + N_PARTIAL]
    delta = [0] * W
    ks = [0] * N_PARTIAL
    for r in range(N_PARTIAL - 2, -1, -1):
        v = mat_vec(Minv, [(d - c) % P for d, c in zip(delta, part[r + 1])])
        ks[r] = (-v[0]) % P
        delta = [0] + v[1:]
    first = [(c - d) % P for c, d in zip(part[0], delta)]
    # k was defined through x+c = y+delta with delta_{r+1} = c_{r+1} + M(delta_r - k_r e0); the
    # sign convention is validated numerically below (naive == fast).
    # --- matrices: M N_{R-1} ... M N_0 = A_{R-1} N_{R-1} ... A_0 N_0 D_0 ----------------------
    D_hat = [[1 if i == j else 0 for j in range(W - 1)] for i in range(W - 1)]
    v_row = M[0][1:]
    rows_v = [None] * N_PARTIAL   # multiplies s[1..] into out[0]
    cols_w = [None] * N_PARTIAL   # multiplies s[0] into out[1..]
    Mhat = [row[1:] for row in M[1:]]
    wcol = [M[i][0] for i in range(1, W)]
    for r in range(N_PARTIAL - 1, -1, -1):
        P_hat = mat_mul(D_hat, Mhat)
        pw = mat_vec(D_hat, wcol)
        P_hat_inv = mat_inv(P_hat)
        # row vector v^T * P_hat^{-1}
        rows_v[r] = [sum(v_row[t] * P_hat_inv[t][j] for t in range(W - 1)) % P for j in range(W - 1)]
        cols_w[r] = pw
        D_hat = P_hat
    init = D_hat  # out[1..] = init * in[1..]
    return dict(first=first, ks=ks, rows_v=rows_v, cols_w=cols_w, init=init, M=M)


def sbox(x):
    return pow(x, 7, P)


def perm_naive(state, rc, M):
    s = [x % P for x in state]
    r = 0
    for _ in range(HALF_FULL):
        s = mat_vec(M, [sbox((a + c) % P) for a, c in zip(s, rc[r])]); r += 1
    for _ in range(N_PARTIAL):
        s = [(a + c) % P for a, c in zip(s, rc[r])]
        s[0] = sbox(s[0])
        s = mat_vec(M, s); r += 1
    for _ in range(HALF_FULL):
        s = mat_vec(M, [sbox((a + c) % P) for a, c in zip(s, rc[r])]); r += 1
    return s


SBOX_INV_EXP = pow(7, -1, P - 1)           # x -> x^7 is a bijection of the field (7 does not divide p - 1): the 7th root is a power


def sbox_inv(x):
    return pow(x, SBOX_INV_EXP, P)


def sbox_inputs(state, rc, M):
    """perm_naive with its trace: (the 30 states right after the round constants -- what the S-boxes of each round read: all twelve
    words in a full round, word 0 in a partial one -- and the output)"""
    s = [x % P for x in state]
    trace = []
    for r in range(N_ROUNDS):
        s = [(a + c) % P for a, c in zip(s, rc[r])]
        trace.append(s[:])
        full = r < HALF_FULL or r >= HALF_FULL + N_PARTIAL
        s = mat_vec(M, [sbox(a) for a in s] if full else [sbox(s[0])] + s[1:])
    return trace, s


def perm_naive_to_input(after_constants, round_, rc, Minv):
    """The input of perm_naive whose state right after the constants of round `round_` is `after_constants`."""
    s = [(a - c) % P for a, c in zip(after_constants, rc[round_])]
    for r in range(round_ - 1, -1, -1):
        s = mat_vec(Minv, s)
        full = r < HALF_FULL or r >= HALF_FULL + N_PARTIAL
        s = [sbox_inv(a) for a in s] if full else [sbox_inv(s[0])] + s[1:]
        s = [(a - c) % P for a, c in zip(s, rc[r])]
    return s


def perm_naive_inverse(out, rc, M):
    """The inverse of perm_naive: the MDS inverse over the field and the 7th root, round by round from the last."""
    Minv = mat_inv(M)
    last = [sbox_inv(a) for a in mat_vec(Minv, [x % P for x in out])]       # the state after the constants of round 29
    return perm_naive_to_input(last, N_ROUNDS - 1, rc, Minv)


def perm_fast(state, rc, T):
    M = T["M"]
    s = [x % P for x in state]
    r = 0
    for _ in range(HALF_FULL):
        s = mat_vec(M, [sbox((a + c) % P) for a, c in zip(s, rc[r])]); r += 1
    s = [(a + c) % P for a, c in zip(s, T["first"])]
    s = [s[0]] + mat_vec(T["init"], s[1:])
    m00 = M[0][0]
    for i in range(N_PARTIAL):
        s0 = (sbox(s[0]) + T["ks"][i]) % P
        d = (s0 * m00 + sum(a * b for a, b in zip(s[1:], T["rows_v"][i]))) % P
        s = [d] + [(s[j] + s0 * T["cols_w"][i][j - 1]) % P for j in range(1, W)]
    r += N_PARTIAL
    for _ in range(HALF_FULL):
        s = mat_vec(M, [sbox((a + c) % P) for a, c in zip(s, rc[r])]); r += 1
    return s


GROUP = 3                                  # partial rounds evaluated per group on the GPU
N_GROUPS = N_PARTIAL // GROUP              # 7 groups cover partial rounds 0..20; the 22nd runs alone


def derive_groups(rc, M):
    """GPU formulation of the partial rounds: three rounds at a time.

    With T the state entering partial round r (round constants already added) and d_j = sbox(a_j) - a_j the change of
    lane 0 in round r+j (a_j = lane 0 before its S-box), linearity of the rest of the round gives
        a_1 = row0(M) T   + d_0 M[0][0]                    + k1
        a_2 = row0(M^2) T + d_0 (M m0)[0] + d_1 M[0][0]     + k2
        T'  = M^3 T + d_0 M^2 m0 + d_1 M m0 + d_2 m0        + K3          (m0 = column 0 of M)
    where k1, k2, K3 collect the round constants of rounds r+1..r+3 pushed through M.  The entries of M^2 and M^3 are
    below 2^13 and 2^21, so every product is still ONE 32 x 32 multiply-add per 32-bit half on the GPU.

    The kernels fold d_0 into the state: V2, V1[0] and V0[0] are column 0 of M^3, M^2[0][0] and M[0][0], so with
    T* = T except T*[0] = sbox(a_0) the three d_0 terms disappear (perm_grouped_folded)."""
    Mi = [[MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]   # plain integers
    imul = lambda A, B: [[sum(A[i][t] * B[t][j] for t in range(W)) for j in range(W)] for i in range(W)]
    M2 = imul(Mi, Mi)
    M3 = imul(M2, Mi)
    assert max(max(r) for r in M2) < 2**13 and max(max(r) for r in M3) < 2**21
    col0 = lambda A: [A[i][0] for i in range(W)]
    G = dict(R1=Mi[0], R2=M2[0], M3=M3, V0=col0(Mi), V1=col0(M2), V2=col0(M3), K=[])
    for g in range(N_GROUPS):
        r = HALF_FULL + GROUP * g
        C1, C2, C3 = rc[r + 1], rc[r + 2], rc[r + 3]
        MC1 = mat_vec(M, C1)
        k2v = [(a + b) % P for a, b in zip(MC1, C2)]
        K3 = [(a + b) % P for a, b in zip(mat_vec(M, k2v), C3)]
        G["K"].append([C1[0], k2v[0]] + K3)
    return G


GROUP4_SPLIT = [4, 4, 4, 4, 4, 3]          # the 23 linear maps behind the S-box layer of full round 3: the MDS layer of that round and
                                           # those of the 22 partial rounds, with the 22 one-word S-boxes between them
assert sum(GROUP4_SPLIT) == N_PARTIAL + 1


def derive_groups4(rc, M):
    """GPU formulation of the partial rounds in groups of g linear maps, g = 4 and 3 (poseidon.cuh psd_partial_group4), folded
    convention: the state s enters and leaves with the constants of its next round added, and word 0 is S-boxed before the maps
    (the head group starts behind the S-box layer of full round 3, where it already is).  With d_0 = 0 by the fold,
        a_j = row0(M^j) s + sum_{0<i<j} (M^(j-i))[0][0] d_i + k_j,   d_j = sbox(a_j) - a_j          (0 < j < g)
        out = M^g s + sum_{0<i<g} col0(M^(g-i)) d_i + K
    Map m of the 23 (m = 0: the MDS layer of full round 3) is followed by the constants of round m + 4; a group whose first map is
    m has c_i = rc[m + i + 3], v_1 = c_1, v_i = M v_(i-1) + c_i, k_j = v_j[0], K = v_g.

    M^4 has 29-bit entries: still one multiply-add per 32-bit half, but the row sums exceed 2^32 (by at most 4 %), so a 64-bit
    accumulator of the last step can wrap -- once: its true value stays below 2^65.  The kernels add the terms in the order of
    group4_last_step below: column 0 of M^4, the largest entry of every row, goes last, and everything before it stays below 2^64,
    so only the carry-out of the final multiply-add has to be kept.  Asserted here for every row."""
    Mi = [[MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]   # plain integers
    imul = lambda A, B: [[sum(A[i][t] * B[t][j] for t in range(W)) for j in range(W)] for i in range(W)]
    M2 = imul(Mi, Mi)
    M3 = imul(M2, Mi)
    M4 = imul(M3, Mi)
    col0 = lambda A: [A[i][0] for i in range(W)]
    assert max(max(r) for r in M4).bit_length() == 29 and max(max(r) for r in M3).bit_length() == 21 and max(col0(M3)).bit_length() == 21
    H = 2**32 - 1                                              # the largest 32-bit half
    for l in range(W):
        before_last = H + H * (Mi[l][0] + sum(M4[l][1:]) + M3[l][0] + M2[l][0])       # K half, d_3, columns 1..11, d_1, d_2
        assert before_last < 2**64, "row %d: a partial sum before the last term can wrap" % l
        assert before_last + H * M4[l][0] < 2**65, "row %d: an accumulator can wrap twice" % l
        assert M4[l][0] == max(M4[l])
    # a_1, a_2, a_3 and the last step of a three-map group cannot wrap at all
    assert H + H * (sum(M3[0]) + M2[0][0] + Mi[0][0]) < 2**63 and H + H * (max(sum(r) for r in M3) + max(col0(M2)) + max(col0(Mi))) < 2**63
    G = dict(split=GROUP4_SPLIT, M1=Mi, M2=M2, M3=M3, M4=M4, K=[], first_map=[])
    m = 0
    for g in GROUP4_SPLIT:
        v = rc[m + 4][:]
        ks = [v[0]]
        for i in range(2, g + 1):
            nxt = rc[m + i + 3] if m + i + 3 < N_ROUNDS else [0] * W
            v = [(a + b) % P for a, b in zip(mat_vec(M, v), nxt)]
            if i < g:
                ks.append(v[0])
        G["K"].append(ks + v)                                  # g - 1 scalars, then K[12]
        G["first_map"].append(m)
        m += g
    return G


def group4_last_step(G, g, s, d, K):
    """The accumulators of the last step of a group of g maps, term by term in the kernels' order: for every output word the lo-half
    and the hi-half sum as integers (not reduced mod 2^64) and whether each wrapped at 2^64.  s: the folded input state (u64 words),
    d: [d_1 .. d_(g-1)].  The order: d_(g-1) col0(M) + K (the multiply-add that carries the constant), columns 1..11 of M^g,
    the remaining d_i, and column 0 of M^g last."""
    pw = {1: G["M1"], 2: G["M2"], 3: G["M3"], 4: G["M4"]}
    Mg = pw[g]
    out = []
    for l in range(W):
        acc = []
        for h in range(2):
            half = lambda x: (x >> (32 * h)) & 0xFFFFFFFF
            a = half(K[l]) + half(d[g - 2]) * pw[1][l][0]
            for i in range(1, W):
                a += half(s[i]) * Mg[l][i]
            for i in range(1, g - 1):
                a += half(d[i - 1]) * pw[g - i][l][0]
            assert a < 2**64, "a partial sum before the last term wrapped"
            a += half(s[0]) * Mg[l][0]
            assert a < 2**65
            acc.append(a)
        out.append((acc[0], acc[1], acc[0] >= 2**64, acc[1] >= 2**64))
    return out


def perm_grouped4(state, rc, M, G, trace=None):
    """The whole permutation as the kernels run it (poseidon.cuh psd_permute_layer): three full rounds, the S-box layer of full round 3,
    the groups of derive_groups4 (the head group takes that round's MDS layer as its first map), the last four full rounds.  State
    words are canonical here.  trace, if a list, receives per group (g, folded input state, [d_i], group4_last_step's result)."""
    mds = lambda s, n: [(a + c) % P for a, c in zip(mat_vec(M, s), rc[n] if n < N_ROUNDS else [0] * W)]
    pw = {1: G["M1"], 2: G["M2"], 3: G["M3"], 4: G["M4"]}
    dot = lambda row, v: sum(a * b for a, b in zip(row, v))
    s = [(a + c) % P for a, c in zip(state, rc[0])]
    for r in range(HALF_FULL - 1):
        s = mds([sbox(a) for a in s], r + 1)
    s = [sbox(a) for a in s]
    for n, g in enumerate(G["split"]):
        ks, K = G["K"][n][:g - 1], G["K"][n][g - 1:]
        if n:
            s = [sbox(s[0])] + s[1:]
        d = []
        for j in range(1, g):
            a = (dot(pw[j][0], s) + sum(pw[j - i][0][0] * d[i - 1] for i in range(1, j)) + ks[j - 1]) % P
            d.append((sbox(a) - a) % P)
        acc = group4_last_step(G, g, s, d, K)
        if trace is not None:
            trace.append((g, s[:], d[:], acc))
        s = [(al + (ah << 32)) % P for al, ah, _, _ in acc]
    r = HALF_FULL + N_PARTIAL
    for _ in range(HALF_FULL):
        s = mds([sbox(a) for a in s], r + 1); r += 1
    return s


MFMA_BIAS = 0x80808080                     # each 32-bit half XOR 0x80808080: bytes b -> signed b - 128 (i8 operands)


def derive_mfma(rc):
    """GPU MDS layer on v_mfma_i32_32x32x32_i8 (poseidon.cuh psd_mds_mfma).

    Every lane multiplies its own state: the B operand of K block q0 is the four 32-bit halves of words 4 q0 .. 4 q0 + 3,
    each XOR 0x80808080, and the 16 result rows of a lane are (output word o of a row block, byte position t): row (o, t)
    = sum_j c_oj (byte_t(half_j) - 128).  The matrix is circulant, so the A operand of (row block R, K block Kb) depends
    only on d = (Kb - R) mod 3, except (0, 0), which also holds MDS_MATRIX_DIAG[0].  A[d][q] packs the coefficients of input
    word q of the K block for the output words o = 0..3 of the row block (byte o); blocks 0..2 by d, block 3 = (0, 0).

    Recombined, sum_t 2^(8t) row(o, t) = sum_j c_oj half_j - rowsum_o 0x80808080, so the constant of the first multiply-add,
    K[n][i] = ((rc_n[i] mod 2^32) + rowsum_i 0x80808080, (rc_n[i] >> 32) + rowsum_i 0x80808080), makes the two 64-bit
    accumulators of output word i exactly those of the VALU layer (psd_mds_then_constants).  Row n = 30: no round constants
    (the last layer)."""
    Mi = [[MDS_CIRC[(c - r) % W] + (MDS_DIAG[r] if r == c else 0) for c in range(W)] for r in range(W)]
    A = []
    for d in range(4):
        for q in range(4):
            w = 0
            for o in range(4):
                c = Mi[o][q] if d == 3 else MDS_CIRC[(4 * d + q - o) % W]
                assert 0 <= c < 128
                w |= c << (8 * o)
            A.append(w)
    rowsum = [sum(r) for r in Mi]
    K = []
    for n in range(N_ROUNDS + 1):
        row = rc[n] if n < N_ROUNDS else [0] * W
        for i in range(W):
            K += [(row[i] & 0xFFFFFFFF) + rowsum[i] * MFMA_BIAS, (row[i] >> 32) + rowsum[i] * MFMA_BIAS]
    return dict(A=A, K=K)


def mds_mfma(s, A, K, n):
    """The MFMA layer's arithmetic in Python, operand by operand: the MDS layer followed by round n's constants (n = 30:
    none), on u64 representatives; returns the (al, ah) pairs, which equal the VALU layer's, and the reduced words."""
    sbyte = lambda x, t: ((x >> (8 * t)) & 0xFF) ^ 0x80
    signed = lambda b: b - 256 if b >= 128 else b
    coef = lambda blk, o, q: (A[4 * blk + q] >> (8 * o)) & 0xFF
    acc = []
    for R in range(3):
        for o in range(4):
            i = 4 * R + o
            pair = []
            for h in range(2):
                tot = K[24 * n + 2 * i + h]
                for t in range(4):
                    row = 0
                    for Kb in range(3):
                        blk = 3 if (R == 0 and Kb == 0) else (Kb - R) % 3
                        for q in range(4):
                            half = (s[4 * Kb + q] >> (32 * h)) & 0xFFFFFFFF
                            row += coef(blk, o, q) * signed(sbyte(half, t))
                    assert -2**31 <= row < 2**31
                    tot += row << (8 * t)
                pair.append(tot % 2**64)
            acc.append(tuple(pair))
    return acc, [(al + (ah << 32)) % P for al, ah in acc]


def perm_grouped_folded(state, rc, M, G):
    """perm_grouped with d_0 folded into the state, as the kernels compute a group (poseidon.cuh psd_partial_group): word 0 becomes
    sbox(a_0) before the three linear maps, and only the d_1 and d_2 corrections remain."""
    dot = lambda row, v: sum(a * b for a, b in zip(row, v)) % P
    mds = lambda s, n: [(a + c) % P for a, c in zip(mat_vec(M, s), rc[n] if n < N_ROUNDS else [0] * W)]
    s = [(a + c) % P for a, c in zip(state, rc[0])]
    r = 0
    for _ in range(HALF_FULL):
        s = mds([sbox(a) for a in s], r + 1); r += 1
    for g in range(N_GROUPS):
        k1, k2, K3 = G["K"][g][0], G["K"][g][1], G["K"][g][2:]
        s = [sbox(s[0])] + s[1:]
        a1 = (dot(G["R1"], s) + k1) % P; d1 = (sbox(a1) - a1) % P
        a2 = (dot(G["R2"], s) + d1 * G["V0"][0] + k2) % P; d2 = (sbox(a2) - a2) % P
        s = [(dot(G["M3"][l], s) + d1 * G["V1"][l] + d2 * G["V0"][l] + K3[l]) % P for l in range(W)]
        r += GROUP
    while r < HALF_FULL + N_PARTIAL:
        s = mds([sbox(s[0])] + s[1:], r + 1); r += 1
    for _ in range(HALF_FULL):
        s = mds([sbox(a) for a in s], r + 1); r += 1
    return s


def perm_grouped(state, rc, M, G):
    s = [x % P for x in state]
    r = 0
    s = [(a + c) % P for a, c in zip(s, rc[0])]
    for _ in range(HALF_FULL):          # T_{r+1} = M sbox(T_r) + rc[r+1]
        s = [(a + c) % P for a, c in zip(mat_vec(M, [sbox(a) for a in s]), rc[r + 1])]; r += 1
    dot = lambda row, v: sum(a * b for a, b in zip(row, v)) % P
    for g in range(N_GROUPS):
        k1, k2, K3 = G["K"][g][0], G["K"][g][1], G["K"][g][2:]
        a0 = s[0]; d0 = (sbox(a0) - a0) % P
        a1 = (dot(G["R1"], s) + d0 * G["V0"][0] + k1) % P; d1 = (sbox(a1) - a1) % P
        a2 = (dot(G["R2"], s) + d0 * G["V1"][0] + d1 * G["V0"][0] + k2) % P; d2 = (sbox(a2) - a2) % P
        s = [(dot(G["M3"][l], s) + d0 * G["V2"][l] + d1 * G["V1"][l] + d2 * G["V0"][l] + K3[l]) % P for l in range(W)]
        r += GROUP
    while r < HALF_FULL + N_PARTIAL:    # leftover partial round(s), textbook form
        s[0] = sbox(s[0])
        s = [(a + c) % P for a, c in zip(mat_vec(M, s), rc[r + 1])]; r += 1
    for _ in range(HALF_FULL):
        nxt = rc[r + 1] if r + 1 < N_ROUNDS else [0] * W
        s = [(a + c) % P for a, c in zip(mat_vec(M, [sbox(a) for a in s]), nxt)]; r += 1
    return s


# Known-answer vectors: plonky2/src/hash/poseidon_goldilocks.rs:449-485 (data).
KATS = [
    ([0] * 12,
     [0x3c18a9786cb0b359, 0xc4055e3364a246c3, 0x7953db0ab48808f4, 0xc71603f33a1144ca,
      0xd7709673896996dc, 0x46a84e87642f44ed, 0xd032648251ee0b3c, 0x1c687363b207df62,
      0xdf8565563e8045fe, 0x40f5b37ff4254dae, 0xd070f637b431067c, 0x1792b1c4342109d7]),
    (list(range(12)),
     [0xd64e1e3efc5b8e9e, 0x53666633020aaa47, 0xd40285597c6a8825, 0x613a4f81e81231d2,
      0x414754bfebd051f0, 0xcb1f8980294a023f, 0x6eb2a9e4d54a9d0f, 0x1902bc3af467e056,
      0xf045d5eafdc6021f, 0xe4150f77caaa3be5, 0xc9bfd01d39b50cce, 0x5c0a27fcb0e1459b]),
    ([P - 1] * 12,
     [0xbe0085cfc57a8357, 0xd95af71847d05c09, 0xcf55a13d33c1c953, 0x95803a74f4530e82,
      0xfcd99eb30a135df1, 0xe095905e913a3029, 0xde0392461b42919b, 0x7d3260e24e81d031,
      0x10d3d0465d9deaa0, 0xa87571083dfc2a47, 0xe18263681e9958f8, 0xe28e96f1ae5e60d3]),
    ([0x8ccbbbea4fe5d2b7, 0xc2af59ee9ec49970, 0x90f7e1a9e658446a, 0xdcc0630a3ab8b1b8,
      0x7ff8256bca20588c, 0x5d99a7ca0c44ecfb, 0x48452b17a70fbee3, 0xeb09d654690b6c88,
      0x4a55d3a39c676a88, 0xc0407a38d2285139, 0xa234bac9356386d1, 0xe1633f2bad98a52f],
     [0xa89280105650c4ec, 0xab542d53860d12ed, 0x5704148e9ccab94f, 0xd3a826d4b62da9f5,
      0x8a7a6ca87892574f, 0xc7017e1cad1a674e, 0x1f06668922318e34, 0xa3b203bc8102676f,
      0xfcc781b0ce382bf2, 0x934c69ff3ed14ba5, 0x504688a5996e8f13, 0x401f3f2ed524a2ba]),
]


def emit(path, rc, T, G, F, G4):
    """Writes <path> (host wrapper, guarded) and <path minus .h>.inc (raw tables behind POSEIDON_TABLE)."""
    def arr(name, vals, per_line=4):
        out = ["POSEIDON_TABLE(%s, %d) = {" % (name, len(vals))]
        for i in range(0, len(vals), per_line):
            out.append("    " + ", ".join("0x%016xULL" % v for v in vals[i:i + per_line]) + ",")
        out.append("};")
        return "\n".join(out)

    def arr32(name, vals, per_line=12):
        out = ["POSEIDON_TABLE32(%s, %d) = {" % (name, len(vals))]
        for i in range(0, len(vals), per_line):
            out.append("    " + ", ".join("%du" % v for v in vals[i:i + per_line]) + ",")
        out.append("};")
        return "\n".join(out)

    flat = lambda rows: [x for row in rows for x in row]
    inc = [
        "// GENERATED by tools/gen_poseidon_constants.py -- do not edit.",
        "// Poseidon over Goldilocks, width 12, rate 8, x^7, 4+22+4 rounds.",
        "// Round constants are data (tools/poseidon_round_constants.txt); the partial-round tables are",
        "// derived by the generator and validated against the reference's known-answer vectors.",
        "// No include guard: the includer defines POSEIDON_TABLE(name, n) (host and device copies).",
        arr("POSEIDON_RC", flat(rc)),
        arr("POSEIDON_MDS_CIRC", MDS_CIRC, 12),
        arr("POSEIDON_MDS_DIAG", MDS_DIAG, 12),
        "// added to the whole state before the partial rounds",
        arr("POSEIDON_PARTIAL_FIRST_RC", T["first"]),
        "// added to state[0] after its s-box in partial round i",
        arr("POSEIDON_PARTIAL_RC", T["ks"]),
        "// dense 11x11 pre-matrix, row-major [in-1][out-1]: out[c] = sum_r in[r] * INIT[r-1][c-1]",
        arr("POSEIDON_PARTIAL_INIT", flat([[T["init"][c][r] for c in range(W - 1)] for r in range(W - 1)])),
        "// per partial round: out[0] = m00*s0 + sum_i s[i]*ROW[r][i-1]",
        arr("POSEIDON_PARTIAL_ROW", flat(T["rows_v"])),
        "// per partial round: out[i] = s[i] + s0*COL[r][i-1]",
        arr("POSEIDON_PARTIAL_COL", flat(T["cols_w"])),
        "// GPU form of the partial rounds, three at a time (derive_groups): row 0 of M^2, M^3 row-major, column 0 of M^2 and",
        "// of M^3 (plain integers < 2^21; V2 serves the unfolded form of the model only: the kernels fold d_0 into the state), and",
        "// per group k1, k2, K3[12] (the round constants pushed through M)",
        arr32("POSEIDON_G3_R2", G["R2"]),
        arr32("POSEIDON_G3_M3", flat(G["M3"])),
        arr32("POSEIDON_G3_V1", G["V1"]),
        arr32("POSEIDON_G3_V2", G["V2"]),
        arr("POSEIDON_G3_K", flat(G["K"])),
        "// GPU form of the permutation's partial rounds (derive_groups4): the 23 linear maps behind the S-box layer of full round 3 in",
        "// groups of %s.  M^4 row-major (29-bit entries; its rows and columns of lower powers are the G3 tables: row 0 of M^3 is the" % "+".join(map(str, G4["split"])),
        "// first row of G3_M3, column 0 of M^3 is G3_V2); per four-map group k1, k2, k3, K[12], then the three-map group's k1, k2, K[12]",
        arr32("POSEIDON_G4_M4", flat(G4["M4"])),
        arr("POSEIDON_G4_K", flat(G4["K"])),
        "// GPU MDS layer on the i8 matrix cores (derive_mfma): A operand coefficients, word 4 d + q = input word q of a K block",
        "// for the output words o = 0..3 of a row block (byte o), d = (K block - row block) mod 3, d = 3: block (0, 0) with the",
        "// diagonal; and per round n (n = 30: no constants) the bias-corrected (k_lo, k_hi) of output word i at 24 n + 2 i",
        arr32("POSEIDON_MDS_I8A", F["A"], 16),
        arr("POSEIDON_MDS_K", F["K"]),
        "// a state whose capacity words 8..11 enter the permutation as zero: their S-boxes of full round 0, sbox(RC[0][8..11])",
        arr("POSEIDON_CAP0_SBOX", [sbox(rc[0][i]) for i in range(8, W)]),
        "",
    ]
    inc_path = path[:-2] + ".inc" if path.endswith(".h") else path + ".inc"
    with open(inc_path, "w") as f:
        f.write("\n".join(inc))
    hdr = [
        "// GENERATED by tools/gen_poseidon_constants.py -- do not edit.",
        "#pragma once",
        "#include <stdint.h>",
        "#define POSEIDON_WIDTH 12",
        "#define POSEIDON_RATE 8",
        "#define POSEIDON_HALF_FULL_ROUNDS 4",
        "#define POSEIDON_PARTIAL_ROUNDS 22",
        "#define POSEIDON_PARTIAL_GROUPS %d" % N_GROUPS,
        "#define POSEIDON_G4_GROUPS %d    /* four-map groups (the first one headed by the MDS layer of full round 3), then one three-map group */" % G4["split"].count(4),
        "#define POSEIDON_TABLE(name, n) static const uint64_t name[n]",
        "#define POSEIDON_TABLE32(name, n) static const uint32_t name[n]",
        '#include "%s"' % os.path.basename(inc_path),
        "#undef POSEIDON_TABLE",
        "#undef POSEIDON_TABLE32",
        "",
    ]
    with open(path, "w") as f:
        f.write("\n".join(hdr))


def main():
    rc = load_round_constants()
    T = derive(rc)
    import random
    rnd = random.Random(1)
    tests = [k[0] for k in KATS] + [[rnd.randrange(P) for _ in range(W)] for _ in range(4)]
    G = derive_groups(rc, T["M"])
    G4 = derive_groups4(rc, T["M"])
    assert G4["split"] == [4] * 5 + [3]                      # what poseidon.cuh psd_permute_layer runs
    for t in tests:
        assert perm_naive(t, rc, T["M"]) == perm_fast(t, rc, T), "fast != naive"
        assert perm_naive(t, rc, T["M"]) == perm_grouped(t, rc, T["M"], G), "grouped != naive"
        assert perm_naive(t, rc, T["M"]) == perm_grouped_folded(t, rc, T["M"], G), "folded groups != naive"
        assert perm_naive(t, rc, T["M"]) == perm_grouped4(t, rc, T["M"], G4), "groups of four != naive"
    for inp, out in KATS:
        assert perm_fast(inp, rc, T) == out, "KAT mismatch"
    F = derive_mfma(rc)
    M = T["M"]
    for t in tests + [[0] * W, [2**64 - 1] * W, [P] * W, [0x7F7F7F7F80808080] * W, [0xFFFFFFFF7F7F7F7F] * W]:
        for n in (1, 17, N_ROUNDS):
            acc, out = mds_mfma(t, F["A"], F["K"], n)
            cst = rc[n] if n < N_ROUNDS else [0] * W
            lo = [x & 0xFFFFFFFF for x in t]; hi = [x >> 32 for x in t]
            assert acc == [(cst[i] % 2**32 + sum(M[i][j] * lo[j] for j in range(W)), (cst[i] >> 32) + sum(M[i][j] * hi[j] for j in range(W)))
                           for i in range(W)], "MFMA accumulators != VALU accumulators"
            assert out == [(a + c) % P for a, c in zip(mat_vec(M, t), cst)], "MFMA layer != M s + rc"
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        HERE, "..", "plonky2_demo_amd", "csrc", "poseidon_constants.h")
    emit(out, rc, T, G, F, G4)
    print("ok: naive==fast==grouped==folded==groups of four on %d inputs, 4 KATs pass, MFMA layer == VALU layer; wrote %s" % (len(tests), os.path.normpath(out)))
    return T


if __name__ == "__main__":
    main()
