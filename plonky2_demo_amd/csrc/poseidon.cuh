// Poseidon-Goldilocks permutation (width 12, rate 8, x^7, 4 + 22 + 4 rounds), device + host.
// Same function as plonky2/src/hash/poseidon.rs:598-609 (pinned by the four known-answer vectors of
// plonky2/src/hash/poseidon_goldilocks.rs:449-485); the sponge / compression wrappers follow
// plonky2/src/hash/hashing.rs:98-146 and plonky2/src/plonk/config.rs:55-66.
//
// GPU (psd_permute under __HIP_DEVICE_COMPILE__): one lane owns one 12-word state (24 VGPRs) and runs the textbook round
// structure; the MDS layer exploits the 6-bit circulant entries: every state word is split into 32-bit halves and the two
// 12-term dot products are accumulated in 64-bit registers without intermediate reduction (v_mad_u64_u32), followed by
// one 96-bit reduction per output word -- the same lazy-reduction idea as poseidon.rs:176-198.
// The linear layers between the S-box layer of full round 3 and full round 26 -- that round's MDS layer and the 22 partial rounds',
// 23 maps with 22 one-word S-boxes between them -- run in groups of 4 + 4 + 4 + 4 + 4 + 3 (psd_partial_group4, psd_partial_group_k):
// six dense maps (five M^4, one M^3) instead of one per round, the S-boxes of a group fed by single rows of M, M^2, M^3.
// Host (Challenger, public_inputs_hash, witness rows, verifier): the factorised "fast" partial rounds of
// poseidon.rs:311-366,399-427 with 128-bit lazy dot products; its tables are derived by tools/gen_poseidon_constants.py.
#pragma once
#include <stdlib.h>
#include "gl64.cuh"
#include "gl64_gfx950.cuh"
#include "poseidon_constants.h"

#if defined(__HIPCC__)
// device copies of the tables (per translation unit, constant address space -> scalar loads)
#define POSEIDON_TABLE(name, n) static __constant__ const uint64_t d_##name[n]
#define POSEIDON_TABLE32(name, n) static __constant__ const uint32_t d_##name[n]
#include "poseidon_constants.inc"
#undef POSEIDON_TABLE
#undef POSEIDON_TABLE32
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define PSD_TAB(name) d_##name
#else
#define PSD_TAB(name) name
#endif

GL_HD gl_t psd_sbox(gl_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const gl_t x2 = glx_mul<false>(x, x), x4 = glx_mul<false>(x2, x2), x3 = glx_mul<false>(x, x2);
    return glx_mul<false>(x3, x4);
#else
    gl_t x2 = gl_sqr(x), x4 = gl_sqr(x2), x3 = gl_mul(x, x2);
    return gl_mul(x3, x4);
#endif
}

// Host formulation (the Challenger, public_inputs_hash, the witness generator's sponge rows, the verifier): 64 x 64 -> 128
// multiplies are native on the CPU, so sums of products are accumulated unreduced in two 128-bit words (the constant is
// split into 32-bit halves: 12 terms of 64 x 32 bits stay below 2^100) and reduced once -- the dependent chain of a dot
// product is one reduction instead of twelve.
typedef unsigned __int128 psd_u128;
struct PsdHostDot { psd_u128 lo = 0, hi = 0; };
inline void psd_host_dot_term(PsdHostDot& d, gl_t s, gl_t c) { d.lo += (psd_u128)s * (uint32_t)c; d.hi += (psd_u128)s * (uint32_t)(c >> 32); }
inline gl_t psd_host_dot_reduce(const PsdHostDot& d) {
    const gl_t h = gl_reduce128((gl_t)d.hi, (gl_t)(d.hi >> 64));            // hi * 2^32
    const gl_t h32 = gl_reduce128(h << 32, h >> 32);
    return gl_add(gl_reduce128((gl_t)d.lo, (gl_t)(d.lo >> 64)), h32);
}
// MDS layer, host formulation (the GPU uses psd_mds_then_constants): the state's 32-bit halves are laid out twice in a
// row so that output r reads a contiguous window -- twelve independent 64-bit accumulators per half, which the compiler
// vectorises (SSE2) and which an AVX2 build of the same loop, selected at run time, does in 64 ns instead of 166.
GL_HD void psd_mds_finish(gl_t (&s)[12], const gl_t* al, const gl_t* ah) {
    for (int r = 0; r < 12; r++) {
        const gl_t l = al[r] + (ah[r] << 32);
        const uint32_t top = (uint32_t)(ah[r] >> 32) + ((l < al[r]) ? 1u : 0u);
        s[r] = gl_reduce96(l, top);
    }
}
GL_HD void psd_mds_portable(gl_t (&s)[12]) {
    const uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    gl_t lo2[24], hi2[24], al[12], ah[12];
    for (int i = 0; i < 12; i++) { lo2[i] = lo2[i + 12] = (uint32_t)s[i]; hi2[i] = hi2[i + 12] = s[i] >> 32; al[i] = 0; ah[i] = 0; }
    for (int i = 0; i < 12; i++) {
        const gl_t c = circ[i];
        for (int r = 0; r < 12; r++) { al[r] += lo2[i + r] * c; ah[r] += hi2[i + r] * c; }    // each sum < 2^41
    }
    al[0] += lo2[0] * 8; ah[0] += hi2[0] * 8;                                                    // MDS_MATRIX_DIAG[0] = 8
    psd_mds_finish(s, al, ah);
}
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) inline void psd_mds_avx2(gl_t (&s)[12]) {
    const uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    gl_t lo2[24], hi2[24];
    for (int i = 0; i < 12; i++) { lo2[i] = lo2[i + 12] = (uint32_t)s[i]; hi2[i] = hi2[i + 12] = s[i] >> 32; }
    __m256i al[3], ah[3];
    for (int k = 0; k < 3; k++) { al[k] = _mm256_setzero_si256(); ah[k] = _mm256_setzero_si256(); }
    for (int i = 0; i < 12; i++) {
        const __m256i c = _mm256_set1_epi64x(circ[i]);
        for (int k = 0; k < 3; k++) {
            al[k] = _mm256_add_epi64(al[k], _mm256_mul_epu32(_mm256_loadu_si256((const __m256i*)(lo2 + i + 4 * k)), c));
            ah[k] = _mm256_add_epi64(ah[k], _mm256_mul_epu32(_mm256_loadu_si256((const __m256i*)(hi2 + i + 4 * k)), c));
        }
    }
    gl_t AL[12], AH[12];
    for (int k = 0; k < 3; k++) { _mm256_storeu_si256((__m256i*)(AL + 4 * k), al[k]); _mm256_storeu_si256((__m256i*)(AH + 4 * k), ah[k]); }
    AL[0] += lo2[0] * 8; AH[0] += hi2[0] * 8;
    psd_mds_finish(s, AL, AH);
}
inline void psd_mds(gl_t (&s)[12]) {
    static const bool have_avx2 = __builtin_cpu_supports("avx2") && !getenv("GL_HOST_MDS_PORTABLE");
    if (have_avx2) psd_mds_avx2(s); else psd_mds_portable(s);
}
#else
GL_HD void psd_mds(gl_t (&s)[12]) { psd_mds_portable(s); }
#endif

GL_HD void psd_full_round(gl_t (&s)[12], int round) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = psd_sbox(gl_add_c(s[i], PSD_TAB(POSEIDON_RC)[12 * round + i]));
    psd_mds(s);
}

GL_HD void psd_partial_rounds(gl_t (&s)[12]) {
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_c(s[i], PSD_TAB(POSEIDON_PARTIAL_FIRST_RC)[i]);
    {
        gl_t t[12];
        t[0] = s[0];
        for (int c = 1; c < 12; c++) {
            PsdHostDot d;
            for (int r = 1; r < 12; r++) psd_host_dot_term(d, s[r], POSEIDON_PARTIAL_INIT[(r - 1) * 11 + (c - 1)]);
            t[c] = psd_host_dot_reduce(d);
        }
        for (int i = 0; i < 12; i++) s[i] = t[i];
    }
    for (int r = 0; r < POSEIDON_PARTIAL_ROUNDS; r++) {
        const gl_t s0 = gl_add_c(psd_sbox(s[0]), POSEIDON_PARTIAL_RC[r]);
        PsdHostDot d;
        psd_host_dot_term(d, s0, 17 + 8);    // MDS[0][0] = circ[0] + diag[0]
        for (int i = 1; i < 12; i++) psd_host_dot_term(d, s[i], POSEIDON_PARTIAL_ROW[r * 11 + i - 1]);
        for (int i = 1; i < 12; i++) s[i] = gl_mul_add(s[i], s0, POSEIDON_PARTIAL_COL[r * 11 + i - 1]);
        s[0] = psd_host_dot_reduce(d);
    }
}

// al + ah 2^32 (al, ah < 2^63) reduced to one word
GL_HD gl_t psd_acc_reduce(gl_t al, gl_t ah) {
#if defined(__HIP_DEVICE_COMPILE__)
    return glx_acc_reduce(al, ah);      // carry add, carry add, multiply-add by EPS with carry, select, add: 5 instructions
#else
    const uint32_t al_hi = (uint32_t)(al >> 32), ah_lo = (uint32_t)ah;
    const uint32_t mid = al_hi + ah_lo;
    const uint32_t top = (uint32_t)(ah >> 32) + (mid < ah_lo ? 1u : 0u);
    return gl_reduce96(((gl_t)mid << 32) | (uint32_t)al, top);
#endif
}

// GPU formulation of the permutation: the TEXTBOOK round structure (poseidon.rs:573-596 `poseidon_naive`: every round is
// constants, S-box, full MDS), not the factorised partial rounds.  On gfx950 a 64 x 64 modular multiply costs ~26 VALU
// instructions while the MDS layer, whose entries are 6-bit constants, is 288 single-instruction multiply-adds plus 12
// reductions: 22 partial rounds as "one S-box + MDS" are ~15 % fewer instructions than "one S-box + 11 modular
// multiply-adds + an 11-term dot product" plus the dense 11 x 11 pre-matrix of the factorised form.  The next round's
// constants ride along as the addend of the first multiply-add of each accumulator, so the constant layer is free.
// Same function (pinned by the reference's known-answer vectors and by fast == naive in the oracle).
// KEEP: the set of output words a layer has to produce, bit i = word i; the words outside it are left unspecified.  What the sponge reads
// of a permutation's last layer: the digest; the capacity, where a full absorb overwrites the rate; everything before a short absorb.
enum : uint32_t { PSD_KEEP_ALL = 0xFFFu, PSD_KEEP_DIGEST = 0x00Fu, PSD_KEEP_CAPACITY = 0xF00u };
template <bool WITH_RC, uint32_t KEEP = PSD_KEEP_ALL>
GL_HD void psd_mds_then_constants(gl_t (&s)[12], const gl_t* __restrict__ rc) {
    // the power-of-two entries are made opaque: otherwise the compiler turns x * 16 into a 64-bit shift-add, which needs
    // the 32-bit operand zero-extended into a register pair first (two extra moves per term); a multiply-add does not
    uint32_t k16 = 16, k2 = 2, k8 = 8;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(k16), "+s"(k2), "+s"(k8));
#endif
    const uint32_t circ[12] = {17, 15, 41, k16, k2, 28, 13, 13, 39, 18, 34, 20};
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
#if defined(__HIP_DEVICE_COMPILE__)
    // three output words at a time: their accumulators are reduced together (glx_acc_reduce3: no wait states)
#pragma unroll
    for (int r0 = 0; r0 < 12; r0 += 3) {
        if (!((KEEP >> r0) & 7u)) continue;          // (a group with a kept word is computed whole: the reduction is one asm block)
        gl_t al[3], ah[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int r = r0 + k;
            // each < (256 + 8 + 1) * 2^32 < 2^41; the round constant is the scalar addend of the first multiply-add (glx_mad_k)
            if (WITH_RC) { const gl_t c = rc[r]; al[k] = glx_mad_k(lo[r], 17u, (uint64_t)(uint32_t)c); ah[k] = glx_mad_k(hi[r], 17u, c >> 32); }
            else { al[k] = (gl_t)lo[r] * 17u; ah[k] = (gl_t)hi[r] * 17u; }
#pragma unroll
            for (int i = 1; i < 12; i++) {
                al[k] += (gl_t)lo[(i + r) % 12] * circ[i];
                ah[k] += (gl_t)hi[(i + r) % 12] * circ[i];
            }
            if (r == 0) { al[k] += (gl_t)lo[0] * k8; ah[k] += (gl_t)hi[0] * k8; }   // MDS_MATRIX_DIAG[0] = 8
        }
        glx_acc_reduce3(al[0], ah[0], al[1], ah[1], al[2], ah[2], s[r0], s[r0 + 1], s[r0 + 2]);
    }
#else
#pragma unroll
    for (int r = 0; r < 12; r++) {
        gl_t al = 0, ah = 0;   // each < (256 + 8 + 1) * 2^32 < 2^41
        if (WITH_RC) { const gl_t c = rc[r]; al = (uint32_t)c; ah = c >> 32; }
#pragma unroll
        for (int i = 0; i < 12; i++) {
            al += (gl_t)lo[(i + r) % 12] * circ[i];
            ah += (gl_t)hi[(i + r) % 12] * circ[i];
        }
        if (r == 0) { al += (gl_t)lo[0] * k8; ah += (gl_t)hi[0] * k8; }   // MDS_MATRIX_DIAG[0] = 8
        s[r] = psd_acc_reduce(al, ah);
    }
#endif
}

// ---- the same layer on the i8 matrix cores (v_mfma_i32_32x32x32_i8) -------------------------------------------------------
// Each lane keeps its own state: the B operand of K block Kb is the four 32-bit halves (lo or hi) of words 4 Kb .. 4 Kb + 3,
// each XOR 0x80808080 (a byte b becomes the signed i8 b - 128; without the bias every byte >= 0x80 would enter as negative).
// The 32 x 32 result has its column on the lane (lane l and l + 32 share column l & 31) and rows 8 (v / 4) + 4 h + (v & 3)
// in register v of lane half h; A is non-zero only in the K set the lane half of the row supplies, so register v = 4 o + t of
// a lane is row (output word o of the row block, byte position t) = sum_j c_oj (byte_t(half_j) - 128) over the lane's OWN
// state, whatever the K order within a lane half.  3 row blocks x 3 K blocks per half: 18 MFMAs.  The circulant makes A depend
// only on (K block - row block) mod 3, plus the (0, 0) block holding MDS_MATRIX_DIAG[0]: 4 A operands of 4 VGPRs.
// Recombined, sum_t 2^(8t) row(o, t) + k = the VALU layer's accumulator exactly (tools/gen_poseidon_constants.py derive_mfma:
// k = the round constant's half + rowsum 0x80808080), so glx_acc_reduce3 returns the same u64 as psd_mds_then_constants.
// An MFMA reads A and B from all 64 lanes whatever EXEC holds: the A operands must be valid in every lane, so the layer runs
// only where the whole wave is active (the hash kernels keep it so: no early exit, stores predicated).
#ifndef PSD_MDS_MFMA
#define PSD_MDS_MFMA 1                  // default MDS layer of the hash kernels (-DPSD_MDS_MFMA=0: the VALU layer)
#endif
#ifndef PSD_GROUP4
#define PSD_GROUP4 1                    // partial rounds of the permutation in groups of four maps (-DPSD_GROUP4=0: three rounds at a time)
#endif
enum { PSD_LAYER_VALU = 0, PSD_LAYER_MFMA = 1, PSD_LAYER_HASH = PSD_MDS_MFMA ? PSD_LAYER_MFMA : PSD_LAYER_VALU };
#if defined(__HIPCC__)
typedef int psd_i32x4 __attribute__((ext_vector_type(4)));
typedef int psd_i32x16 __attribute__((ext_vector_type(16)));
struct PsdMfmaA { psd_i32x4 blk[4]; };     // blk[d]: d = (K block - row block) mod 3; blk[3]: the (0, 0) block
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// the lane's A operands: row r = lane & 31 is (o = r >> 3, t = r & 3) and lives in lane half (r >> 2) & 1; its K entries are
// the coefficient of input word q at byte t of register q (the B operand's layout), zero in the other lane half
__device__ __forceinline__ PsdMfmaA psd_mfma_a() {
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)), r = lane & 31;
    const bool mine = ((r >> 2) & 1) == (lane >> 5);
    const uint32_t o8 = 8 * (r >> 3), t8 = 8 * (r & 3);
    PsdMfmaA A;
#pragma unroll
    for (int d = 0; d < 4; d++)
#pragma unroll
        for (int q = 0; q < 4; q++) A.blk[d][q] = mine ? (int)(((d_POSEIDON_MDS_I8A[4 * d + q] >> o8) & 0xFFu) << t8) : 0;
    return A;
}
// M s + the constants of round n (kk = d_POSEIDON_MDS_K + 24 n, n = 30: none) on the matrix cores; bit-identical to
// psd_mds_then_constants for any u64 representatives
// KEEP (PSD_KEEP_*): the output words to produce; the others are left unspecified (here: undefined values, see below).  A row block without a kept word runs no MFMA,
// a word that is not kept no recombination and no reduction (the reductions' asm blocks are opaque: the compiler drops none by itself).
template <uint32_t KEEP>
__device__ __forceinline__ void psd_mds_mfma(gl_t (&s)[12], const gl_t* __restrict__ kk, const PsdMfmaA& A) {
    psd_i32x4 bl[3], bh[3];
#pragma unroll
    for (int kb = 0; kb < 3; kb++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            bl[kb][q] = (int)((uint32_t)s[4 * kb + q] ^ 0x80808080u);
            bh[kb][q] = (int)((uint32_t)(s[4 * kb + q] >> 32) ^ 0x80808080u);
        }
    // a word that is not kept dies here (an undefined value, no instruction): where the caller's next write to it is conditional -- the
    // sponge's absorb -- the old word would otherwise stay in its registers through the layer
#pragma unroll
    for (int i = 0; i < 12; i++)
        if (!((KEEP >> i) & 1u)) asm("" : "=v"(s[i]));
    // opaque multipliers: the recombination stays one v_mad_i64_i32 per byte position (a known power of two becomes a
    // sign-extension and a 64-bit shift-add); `one` in a VGPR leaves the one scalar operand to the 64-bit constant k
    int32_t one = 1, m8 = 1 << 8, m16 = 1 << 16, m24 = 1 << 24;
    asm volatile("" : "+v"(one), "+s"(m8), "+s"(m16), "+s"(m24));
    gl_t acc[2][12];                       // [half][output word]: the VALU layer's al, ah
#pragma unroll
    for (int rb = 0; rb < 3; rb++) {
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            if (!((KEEP >> (4 * rb)) & 0xFu)) continue;
            // one accumulator chain at a time (16 VGPRs): the scheduler would otherwise start all six at once
            __builtin_amdgcn_sched_barrier(0);
            psd_i32x16 d = {};
#pragma unroll
            for (int kb = 0; kb < 3; kb++)
                d = __builtin_amdgcn_mfma_i32_32x32x32_i8((rb == 0 && kb == 0) ? A.blk[3] : A.blk[(kb - rb + 3) % 3], hf ? bh[kb] : bl[kb], d, 0, 0, 0);
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int i = 4 * rb + o;
                if (!((KEEP >> i) & 1u)) continue;
                int64_t x = (int64_t)d[4 * o] * one + (int64_t)kk[2 * i + hf];
                x += (int64_t)d[4 * o + 1] * m8;
                x += (int64_t)d[4 * o + 2] * m16;
                x += (int64_t)d[4 * o + 3] * m24;
                acc[hf][i] = (gl_t)x;
            }
        }
        // reduce the groups of three this row block completes (outputs 0-2 | 3-5 | 6-8, 9-11): three at once where all are kept,
        // one by one otherwise
#pragma unroll
        for (int r0 = 3 * rb; r0 < 4 * rb + 2; r0 += 3) {
            if (((KEEP >> r0) & 7u) == 7u)
                glx_acc_reduce3(acc[0][r0], acc[1][r0], acc[0][r0 + 1], acc[1][r0 + 1], acc[0][r0 + 2], acc[1][r0 + 2], s[r0], s[r0 + 1], s[r0 + 2]);
            else {
#pragma unroll
                for (int r = r0; r < r0 + 3; r++)
                    if ((KEEP >> r) & 1u) s[r] = glx_acc_reduce(acc[0][r], acc[1][r]);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}
#endif

// M[r][c] of the MDS matrix (circulant + diag(8, 0, ...)), compile-time after unrolling
GL_HD constexpr uint32_t psd_mds_entry(int r, int c) {
    constexpr uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    return circ[(c - r + 12) % 12] + ((r == 0 && c == 0) ? 8u : 0u);
}
// cap0 (wave-uniform): the layer is that of full round 0 and the capacity words entered the permutation as zero, so the S-boxes of
// words 9..11 are the tabled sbox(RC[0][9..11]) and their triple is skipped (word 8 rides in the triple of words 6 and 7)
GL_HD void psd_sbox_all(gl_t (&s)[12], bool cap0 = false) {
#if defined(__HIP_DEVICE_COMPILE__)
    // x^7 = (x * x^2) * x^4, three words at a time: glx_mul3 interleaves three independent products so that its carry chains
    // need no wait states (12 instructions per product; each call tests its three borrow masks on the scalar unit and leaves
    // the rare subtracting side of the fix-up to a cold block: 16 wave-uniform branches per layer, none taken on ordinary data)
#pragma unroll
    for (int k = 0; k < 12; k += 3) {
        if (k == 9 && cap0) {
#pragma unroll
            for (int i = 9; i < 12; i++) s[i] = d_POSEIDON_CAP0_SBOX[i - 8];
            continue;
        }
        gl_t a2, b2, c2, a4, b4, c4, a3, b3, c3;
        glx_mul3<false>(s[k], s[k], s[k + 1], s[k + 1], s[k + 2], s[k + 2], a2, b2, c2);
        glx_mul3<false>(a2, a2, b2, b2, c2, c2, a4, b4, c4);
        glx_mul3<false>(s[k], a2, s[k + 1], b2, s[k + 2], c2, a3, b3, c3);
        glx_mul3<false>(a3, a4, b3, b4, c3, c4, s[k], s[k + 1], s[k + 2]);
    }
#else
    for (int i = 0; i < 12; i++) s[i] = psd_sbox(s[i]);
#endif
}
#if defined(__HIPCC__)
// Three partial rounds at once (tools/gen_poseidon_constants.py derive_groups): with d_j = sbox(x_j) - a_j the change of lane
// 0 in round j of the group (a_j = lane 0 entering its S-box), everything else is linear, so lane 0 of the next two rounds
// needs only row 0 of M and of M^2 applied to the group's input state, and the state after the group is M^3 (entries
// < 2^21: still one multiply-add per 32-bit half) applied to it plus rank-one corrections.  The first correction is folded
// into the state: the d_0 terms are d_0 times column 0 of M, M^2 and M^3, so word 0 is replaced by sbox(x_0) before the three
// linear maps and only d_1 and d_2 remain.  `s` enters and leaves with the round constants of its next round already added.
// SUBST = false: x_j = a_j (the permutation).  SUBST = true: x_j = in[j], the PoseidonGate's S-box input wires, and a[j]
// returns the computed a_j for the constraint a_j - in[j] (gates/poseidon.rs:165-189).
// K: the group's k1, k2, K3[12] (psd_partial_group: group g of the three-round grouping; the permutation's last, three-map group
// passes its own constants)
template <bool SUBST>
__device__ __forceinline__ void psd_partial_group_k(gl_t (&s)[12], const gl_t* __restrict__ K, const gl_t* in, gl_t* a) {
    // the matrix constants are re-read (scalar loads) in every group: hoisted out of the loop they exceed the SGPR file
    // and get parked in VGPR lanes (250 v_readlane per group)
    uint32_t z = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(z));
#endif
    const uint32_t* __restrict__ R2 = d_POSEIDON_G3_R2 + z;
    const uint32_t* __restrict__ V1 = d_POSEIDON_G3_V1 + z;
    a[0] = s[0];
    s[0] = psd_sbox(SUBST ? in[0] : s[0]);
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
    gl_t al = glx_mad_k(lo[0], psd_mds_entry(0, 0), (uint64_t)(uint32_t)K[0]), ah = glx_mad_k(hi[0], psd_mds_entry(0, 0), K[0] >> 32);
#pragma unroll
    for (int i = 1; i < 12; i++) { al = glx_mac_c(al, lo[i], psd_mds_entry(0, i)); ah = glx_mac_c(ah, hi[i], psd_mds_entry(0, i)); }
    const gl_t a1 = psd_acc_reduce(al, ah);
    a[1] = a1;
    const gl_t d1 = gl_sub(psd_sbox(SUBST ? in[1] : a1), a1);
    const uint32_t d1l = (uint32_t)d1, d1h = (uint32_t)(d1 >> 32);
    al = glx_mad_k(d1l, psd_mds_entry(0, 0), (uint64_t)(uint32_t)K[1]); ah = glx_mad_k(d1h, psd_mds_entry(0, 0), K[1] >> 32);   // (inline-constant coefficient first)
#pragma unroll
    for (int i = 0; i < 12; i++) { const uint32_t c = R2[i]; al += (gl_t)lo[i] * c; ah += (gl_t)hi[i] * c; }
    const gl_t a2 = psd_acc_reduce(al, ah);
    a[2] = a2;
    const gl_t d2 = gl_sub(psd_sbox(SUBST ? in[2] : a2), a2);
    const uint32_t d2l = (uint32_t)d2, d2h = (uint32_t)(d2 >> 32);
    const uint32_t* __restrict__ M3 = d_POSEIDON_G3_M3 + z;
#pragma unroll
    for (int l0 = 0; l0 < 12; l0 += 3) {
        gl_t xl[3], xh[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int l = l0 + k;
            // the term with a compile-time (inline-constant) coefficient goes first: its multiply-add takes the round constant as
            // a scalar 64-bit addend, which a multiply-add with a scalar coefficient cannot (one scalar operand per instruction)
            // -- otherwise every accumulator starts with two register moves
            xl[k] = glx_mad_k(d2l, psd_mds_entry(l, 0), (uint64_t)(uint32_t)K[2 + l]); xh[k] = glx_mad_k(d2h, psd_mds_entry(l, 0), K[2 + l] >> 32);
#pragma unroll
            for (int i = 0; i < 12; i++) { const uint32_t c = M3[12 * l + i]; xl[k] += (gl_t)lo[i] * c; xh[k] += (gl_t)hi[i] * c; }
            { const uint32_t c = V1[l]; xl[k] += (gl_t)d1l * c; xh[k] += (gl_t)d1h * c; }
        }
        glx_acc_reduce3(xl[0], xh[0], xl[1], xh[1], xl[2], xh[2], s[l0], s[l0 + 1], s[l0 + 2]);
    }
}
template <bool SUBST>
__device__ __forceinline__ void psd_partial_group(gl_t (&s)[12], int g, const gl_t* in, gl_t* a) {
    psd_partial_group_k<SUBST>(s, d_POSEIDON_G3_K + 14 * g, in, a);
}

// Four linear maps at once (tools/gen_poseidon_constants.py derive_groups4, perm_grouped4), the permutation only.  Same folded
// convention: `s` enters and leaves with the constants of its next round added and word 0 is S-boxed before the maps -- by this
// function, except in the head group (fold = false), which starts right behind the S-box layer of full round 3 and takes that
// round's MDS layer as its first map.  a_1, a_2, a_3 need row 0 of M, M^2, M^3; the state after the group is M^4 s plus d_1, d_2, d_3
// times column 0 of M^3, M^2, M.  M^4 has 29-bit entries, still one multiply-add per 32-bit half, but its row sums are up to
// 1.04 2^32: an accumulator of the last step can wrap, once (its true value is below 2^65).  The terms are ordered so that only the
// last multiply-add can carry -- d_3 col0(M) + K first, columns 1..11, d_1, d_2, and column 0 of M^4, the largest entry of every
// row, last (the generator asserts that everything before it is below 2^64) -- and glx_acc_reduce3w takes its carry-out.
__device__ __forceinline__ void psd_partial_group4(gl_t (&s)[12], const gl_t* __restrict__ K, bool fold) {
    uint32_t z = 0;
    asm volatile("" : "+s"(z));            // the matrix constants are re-read in every group (psd_partial_group_k)
    const uint32_t* __restrict__ R2 = d_POSEIDON_G3_R2 + z;
    const uint32_t* __restrict__ R3 = d_POSEIDON_G3_M3 + z;        // row 0 of M^3
    const uint32_t* __restrict__ V2 = d_POSEIDON_G3_V1 + z;        // column 0 of M^2
    const uint32_t* __restrict__ V3 = d_POSEIDON_G3_V2 + z;        // column 0 of M^3
    if (fold) s[0] = psd_sbox(s[0]);       // wave-uniform
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int i = 0; i < 12; i++) { lo[i] = (uint32_t)s[i]; hi[i] = (uint32_t)(s[i] >> 32); }
    gl_t al = glx_mad_k(lo[0], psd_mds_entry(0, 0), (uint64_t)(uint32_t)K[0]), ah = glx_mad_k(hi[0], psd_mds_entry(0, 0), K[0] >> 32);
#pragma unroll
    for (int i = 1; i < 12; i++) { al = glx_mac_c(al, lo[i], psd_mds_entry(0, i)); ah = glx_mac_c(ah, hi[i], psd_mds_entry(0, i)); }
    const gl_t a1 = psd_acc_reduce(al, ah);
    const gl_t d1 = gl_sub(psd_sbox(a1), a1);
    const uint32_t d1l = (uint32_t)d1, d1h = (uint32_t)(d1 >> 32);
    al = glx_mad_k(d1l, psd_mds_entry(0, 0), (uint64_t)(uint32_t)K[1]); ah = glx_mad_k(d1h, psd_mds_entry(0, 0), K[1] >> 32);
#pragma unroll
    for (int i = 0; i < 12; i++) { const uint32_t c = R2[i]; al += (gl_t)lo[i] * c; ah += (gl_t)hi[i] * c; }
    const gl_t a2 = psd_acc_reduce(al, ah);
    const gl_t d2 = gl_sub(psd_sbox(a2), a2);
    const uint32_t d2l = (uint32_t)d2, d2h = (uint32_t)(d2 >> 32);
    al = glx_mad_k(d2l, psd_mds_entry(0, 0), (uint64_t)(uint32_t)K[2]); ah = glx_mad_k(d2h, psd_mds_entry(0, 0), K[2] >> 32);
#pragma unroll
    for (int i = 0; i < 12; i++) { const uint32_t c = R3[i]; al += (gl_t)lo[i] * c; ah += (gl_t)hi[i] * c; }
    { const uint32_t c = V2[0]; al += (gl_t)d1l * c; ah += (gl_t)d1h * c; }           // below 2^63 in all: 21-bit entries
    const gl_t a3 = psd_acc_reduce(al, ah);
    const gl_t d3 = gl_sub(psd_sbox(a3), a3);
    const uint32_t d3l = (uint32_t)d3, d3h = (uint32_t)(d3 >> 32);
    const uint32_t* __restrict__ M4 = d_POSEIDON_G4_M4 + z;
#pragma unroll
    for (int l0 = 0; l0 < 12; l0 += 3) {
        gl_t xl[3], xh[3];
        uint64_t wl[3], wh[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int l = l0 + k;
            xl[k] = glx_mad_k(d3l, psd_mds_entry(l, 0), (uint64_t)(uint32_t)K[3 + l]); xh[k] = glx_mad_k(d3h, psd_mds_entry(l, 0), K[3 + l] >> 32);
#pragma unroll
            for (int i = 1; i < 12; i++) { const uint32_t c = M4[12 * l + i]; xl[k] += (gl_t)lo[i] * c; xh[k] += (gl_t)hi[i] * c; }
            { const uint32_t c = V3[l]; xl[k] += (gl_t)d1l * c; xh[k] += (gl_t)d1h * c; }
            { const uint32_t c = V2[l]; xl[k] += (gl_t)d2l * c; xh[k] += (gl_t)d2h * c; }
            { const uint32_t c = M4[12 * l]; xl[k] = glx_mac_co(xl[k], lo[0], c, wl[k]); xh[k] = glx_mac_co(xh[k], hi[0], c, wh[k]); }
        }
        glx_acc_reduce3w(xl[0], xh[0], wl[0], wh[0], xl[1], xh[1], wl[1], wh[1], xl[2], xh[2], wl[2], wh[2], s[l0], s[l0 + 1], s[l0 + 2]);
    }
}
#endif

#if defined(__HIP_DEVICE_COMPILE__)
// the MDS layer of round n - 1 followed by the constants of round n (n = 30: none), on the chosen unit; KEEP: the words to produce
template <int LAYER, bool WITH_RC, uint32_t KEEP = PSD_KEEP_ALL>
__device__ __forceinline__ void psd_mds_layer(gl_t (&s)[12], int n, const PsdMfmaA& A) {
    if constexpr (LAYER == PSD_LAYER_MFMA) psd_mds_mfma<KEEP>(s, d_POSEIDON_MDS_K + 24 * (WITH_RC ? n : 8 + POSEIDON_PARTIAL_ROUNDS), A);
    else psd_mds_then_constants<WITH_RC, KEEP>(s, WITH_RC ? d_POSEIDON_RC + 12 * n : nullptr);
}
// The permutation up to and including the S-box layer of its last round: the last MDS layer is the caller's (psd_permute_layer,
// psd_sponge_permute), which knows the words that are read.  cap0 (wave-uniform): words 8..11 enter as zero (psd_sbox_all).
// LAYER = PSD_LAYER_MFMA: every lane of the wave must be active (psd_mds_mfma)
template <int LAYER>
__device__ __forceinline__ void psd_permute_rounds(gl_t (&s)[12], const PsdMfmaA& A, bool cap0) {
    const gl_t* __restrict__ rc = d_POSEIDON_RC;
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = gl_add_c(s[i], rc[i]);
#if PSD_GROUP4
    // three full rounds and the S-box layer of the fourth; its MDS layer and those of the 22 partial rounds are 23 linear maps with
    // 22 one-word S-boxes between them, run as 4 + 4 + 4 + 4 + 4 + 3 (six dense maps): five groups of four, one of three
#pragma unroll 1
    for (int r = 0; r < 4; r++) { psd_sbox_all(s, cap0 && r == 0); if (r < 3) psd_mds_layer<LAYER, true>(s, r + 1, A); }
#pragma unroll 1
    for (int g = 0; g < POSEIDON_G4_GROUPS; g++) psd_partial_group4(s, d_POSEIDON_G4_K + 15 * g, g != 0);
    { gl_t a[3]; psd_partial_group_k<false>(s, d_POSEIDON_G4_K + 15 * POSEIDON_G4_GROUPS, nullptr, a); }
#else
#pragma unroll 1
    for (int r = 0; r < 4; r++) { psd_sbox_all(s, cap0 && r == 0); psd_mds_layer<LAYER, true>(s, r + 1, A); }
#pragma unroll 1
    for (int g = 0; g < POSEIDON_PARTIAL_GROUPS; g++) { gl_t a[3]; psd_partial_group<false>(s, g, nullptr, a); }
#pragma unroll 1
    for (int r = 4 + 3 * POSEIDON_PARTIAL_GROUPS; r < 4 + POSEIDON_PARTIAL_ROUNDS; r++) { s[0] = psd_sbox(s[0]); psd_mds_layer<LAYER, true>(s, r + 1, A); }
#endif
#pragma unroll 1
    for (int r = 4 + POSEIDON_PARTIAL_ROUNDS; r < 7 + POSEIDON_PARTIAL_ROUNDS; r++) { psd_sbox_all(s); psd_mds_layer<LAYER, true>(s, r + 1, A); }
    psd_sbox_all(s);
}
// One permutation of which the words in KEEP are read afterwards; CAP0: words 8..11 are zero on entry (two_to_one, a sponge's first block)
template <int LAYER, uint32_t KEEP = PSD_KEEP_ALL, bool CAP0 = false>
__device__ __forceinline__ void psd_permute_layer(gl_t (&s)[12]) {
    PsdMfmaA A;
    if constexpr (LAYER == PSD_LAYER_MFMA) A = psd_mfma_a();
    psd_permute_rounds<LAYER>(s, A, CAP0);
    psd_mds_layer<LAYER, false, KEEP>(s, 0, A);
}
// One permutation of an overwrite-mode sponge (hashing.rs:117-131) whose capacity started as zero.  first: the sponge's first block;
// next: the number of words the next absorb overwrites -- 8: only the capacity is read; 1..7, a short last block: words next..11 are,
// and the whole layer is run (one copy of the layer for every length would be seven more); 0: the last permutation, the digest is
// read.  Both are wave-uniform, so the round body is there once and only the last layer has three forms.
template <int LAYER>
__device__ __forceinline__ void psd_sponge_permute(gl_t (&s)[12], bool first, uint32_t next) {
    PsdMfmaA A;
    if constexpr (LAYER == PSD_LAYER_MFMA) A = psd_mfma_a();
    psd_permute_rounds<LAYER>(s, A, first);
    if (next == 8) psd_mds_layer<LAYER, false, PSD_KEEP_CAPACITY>(s, 0, A);
    else if (next == 0) psd_mds_layer<LAYER, false, PSD_KEEP_DIGEST>(s, 0, A);
    else psd_mds_layer<LAYER, false>(s, 0, A);
}
// any EXEC mask: the VALU layer (the hash kernels call psd_permute_layer<PSD_LAYER_HASH> with the whole wave active)
GL_HD void psd_permute(gl_t (&s)[12]) { psd_permute_layer<PSD_LAYER_VALU>(s); }
#else
#if defined(__HIPCC__)
template <int LAYER, uint32_t KEEP = PSD_KEEP_ALL, bool CAP0 = false>
__device__ void psd_permute_layer(gl_t (&s)[12]);       // host pass of a .hip file: kernels that call it must still parse
template <int LAYER>
__device__ void psd_sponge_permute(gl_t (&s)[12], bool first, uint32_t next);
#endif
GL_HD void psd_permute(gl_t (&s)[12]) {         // host formulation (GL_HD only so that kernels parse in the host pass)
    for (int r = 0; r < 4; r++) psd_full_round(s, r);
    psd_partial_rounds(s);
    for (int r = 0; r < 4; r++) psd_full_round(s, 4 + POSEIDON_PARTIAL_ROUNDS + r);
}
#endif

#if defined(__HIPCC__)
// Cooperative permutation for LATENCY-bound launches (the upper levels of a Merkle tree, the small FRI trees): 16 lanes
// share one state, lane l < 12 holds word l, so the 12 S-boxes of a full round run side by side and the MDS layer is 22
// cross-lane reads (ds_bpermute) plus 24 multiply-adds per lane.  The dependent chain of a permutation shrinks from
// ~23 k to ~5 k instructions; three quarters of the lanes' issue slots are idle, so it only pays when the launch could
// not fill the chip anyway.  `l` = lane & 15; lanes 12..15 carry zeros and mirror word 0's control flow.
__device__ __forceinline__ gl_t psd_coop_permute(gl_t s, const int l) {
    const uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    const gl_t* __restrict__ rc = d_POSEIDON_RC;
    const int lc = l < 12 ? l : 0;
    const int lane = (int)(threadIdx.x & 63), row = lane & ~15;
    s = gl_add_c(s, rc[lc]);
#pragma unroll 1
    for (int r = 0; r < 8 + POSEIDON_PARTIAL_ROUNDS; r++) {
        const bool full = r < 4 || r >= 4 + POSEIDON_PARTIAL_ROUNDS;
        if (full || l == 0) s = psd_sbox(s);
        const uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
        gl_t al = 0, ah = 0;
        if (r + 1 < 8 + POSEIDON_PARTIAL_ROUNDS) { const gl_t c = rc[12 * (r + 1) + lc]; al = (uint32_t)c; ah = c >> 32; }
        al = glx_mac_c(al, lo, 17u); ah = glx_mac_c(ah, hi, 17u);      // circ[0]; multiply-adds, not shift-adds (glx_mac_c)
#pragma unroll
        for (int i = 1; i < 12; i++) {
            int src = lc + i; src -= (src >= 12) ? 12 : 0;
            const int addr = (row + src) << 2;
            const uint32_t lo_i = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)lo);
            const uint32_t hi_i = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)hi);
            al = glx_mac_c(al, lo_i, circ[i]); ah = glx_mac_c(ah, hi_i, circ[i]);
        }
        if (l == 0) { al += (gl_t)lo * 8; ah += (gl_t)hi * 8; }   // MDS_MATRIX_DIAG[0] = 8
        s = psd_acc_reduce(al, ah);
        if (l >= 12) s = 0;
    }
    return s;
}
#endif

// two_to_one (hashing.rs:98-115): permute([l, r, 0,0,0,0])[0..4]
GL_HD void psd_two_to_one(const gl_t* l, const gl_t* r, gl_t* out) {
    gl_t s[12];
#pragma unroll
    for (int i = 0; i < 4; i++) { s[i] = l[i]; s[4 + i] = r[i]; s[8 + i] = 0; }
    psd_permute(s);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = gl_canon(s[i]);
}
