// Keccak-256 for KeccakGoldilocksConfig (plonky2/src/plonk/config.rs:110-118: Hasher = KeccakHash<25>, InnerHasher = PoseidonHash;
// plonky2/src/hash/keccak.rs), for gfx950 kernels and for the host-side driver: ONE implementation, compiled for both.
//
// A BytesHash<25> travels in the four-u64 slot of a HashOut: its 25 bytes little-endian in words 0..3, the top 7 bytes of word 3 zero.
//
// Keccak-f[1600] works on the state as 25 lanes of two 32-bit halves with static indices only, written for the gfx950 instruction
// count: every three-input boolean step is one v_bitop3_b32 (the five-way column parity in two, theta's a ^ C ^ rot(C) in one with
// truth table 0x96, chi's a ^ (~b & c) in one with 0xd2), a 64-bit rotate is two v_alignbit_b32 (a rotate by 32 is a renaming), iota is
// an xor with a constant.  One round is 120 + 54 + 4 + 2 instructions; see DESIGN.md section 13 for the counted disassembly.
// The padding is the ORIGINAL Keccak one (domain byte 0x01, final bit 0x80), as the keccak-hash crate computes it -- not SHA-3's 0x06.
#pragma once
#include "gl64.cuh"

#define GL_HASHER_POSEIDON 0u
#define GL_HASHER_KECCAK 1u
#define KCK_RATE_WORDS 17          // rate 136 bytes
#define KCK_HASH_BYTES 25          // KeccakHash<25>

// ---- three-input boolean functions and the 64-bit rotate on halves ----
#if defined(__HIP_DEVICE_COMPILE__)
GL_HD uint32_t kck_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
GL_HD uint32_t kck_chi(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xd2); }      // a ^ (~b & c)
// ((hi : lo) >> sh) & 0xffffffff, 0 < sh < 32
GL_HD uint32_t kck_align(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
#else
GL_HD uint32_t kck_xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
GL_HD uint32_t kck_chi(uint32_t a, uint32_t b, uint32_t c) { return a ^ (~b & c); }
GL_HD uint32_t kck_align(uint32_t hi, uint32_t lo, uint32_t sh) { return (hi << (32 - sh)) | (lo >> sh); }
#endif

struct kck_state { uint32_t lo[25], hi[25]; };      // lane x + 5 y

// (olo, ohi) = rotl64((lo, hi), R), R a compile-time constant
template <int R>
GL_HD void kck_rotl(uint32_t lo, uint32_t hi, uint32_t& olo, uint32_t& ohi) {
    if (R == 0) { olo = lo; ohi = hi; }
    else if (R == 32) { olo = hi; ohi = lo; }
    else if (R < 32) { olo = kck_align(lo, hi, 32 - R); ohi = kck_align(hi, lo, 32 - R); }
    else { olo = kck_align(hi, lo, 64 - R); ohi = kck_align(lo, hi, 64 - R); }
}

// one row of chi over the five lanes b0..b4 into lanes Y..Y+4 of the state
#define KCK_CHI_ROW(Y)                                                                   \
    s.lo[Y + 0] = kck_chi(bl0, bl1, bl2); s.hi[Y + 0] = kck_chi(bh0, bh1, bh2);          \
    s.lo[Y + 1] = kck_chi(bl1, bl2, bl3); s.hi[Y + 1] = kck_chi(bh1, bh2, bh3);          \
    s.lo[Y + 2] = kck_chi(bl2, bl3, bl4); s.hi[Y + 2] = kck_chi(bh2, bh3, bh4);          \
    s.lo[Y + 3] = kck_chi(bl3, bl4, bl0); s.hi[Y + 3] = kck_chi(bh3, bh4, bh0);          \
    s.lo[Y + 4] = kck_chi(bl4, bl0, bl1); s.hi[Y + 4] = kck_chi(bh4, bh0, bh1);
// B[k] = rotl(A[src] ^ D[src % 5], R): theta's xor (one bitop3 with the two halves of D) and rho/pi
#define KCK_B(K, SRC, R)                                                                                       \
    kck_rotl<R>(kck_xor3(a.lo[SRC], dal[(SRC) % 5], dbl[(SRC) % 5]), kck_xor3(a.hi[SRC], dah[(SRC) % 5], dbh[(SRC) % 5]), bl##K, bh##K);

// one round; theta's D[x] = C[x-1] ^ rotl(C[x+1], 1) is never formed: A ^ D is A ^ C[x-1] ^ rotl(C[x+1], 1), one three-input xor
GL_HD void kck_round(kck_state& s, uint32_t rc_lo, uint32_t rc_hi) {
    const kck_state a = s;
    uint32_t cl[5], ch[5], dal[5], dah[5], dbl[5], dbh[5];
#pragma unroll
    for (int x = 0; x < 5; x++) {
        cl[x] = kck_xor3(kck_xor3(a.lo[x], a.lo[x + 5], a.lo[x + 10]), a.lo[x + 15], a.lo[x + 20]);
        ch[x] = kck_xor3(kck_xor3(a.hi[x], a.hi[x + 5], a.hi[x + 10]), a.hi[x + 15], a.hi[x + 20]);
    }
#pragma unroll
    for (int x = 0; x < 5; x++) {
        dal[x] = cl[(x + 4) % 5]; dah[x] = ch[(x + 4) % 5];
        kck_rotl<1>(cl[(x + 1) % 5], ch[(x + 1) % 5], dbl[x], dbh[x]);
    }
    uint32_t bl0, bl1, bl2, bl3, bl4, bh0, bh1, bh2, bh3, bh4;
    // row y of the output needs B[x + 5 y] = rotl(A'[(x + 3 y) % 5 + 5 x], r); the rows are produced one after the other so that
    // only five B lanes are alive at a time
    KCK_B(0, 0, 0) KCK_B(1, 6, 44) KCK_B(2, 12, 43) KCK_B(3, 18, 21) KCK_B(4, 24, 14)
    KCK_CHI_ROW(0)
    s.lo[0] ^= rc_lo; s.hi[0] ^= rc_hi;                                  // iota
    KCK_B(0, 3, 28) KCK_B(1, 9, 20) KCK_B(2, 10, 3) KCK_B(3, 16, 45) KCK_B(4, 22, 61)
    KCK_CHI_ROW(5)
    KCK_B(0, 1, 1) KCK_B(1, 7, 6) KCK_B(2, 13, 25) KCK_B(3, 19, 8) KCK_B(4, 20, 18)
    KCK_CHI_ROW(10)
    KCK_B(0, 4, 27) KCK_B(1, 5, 36) KCK_B(2, 11, 10) KCK_B(3, 17, 15) KCK_B(4, 23, 56)
    KCK_CHI_ROW(15)
    KCK_B(0, 2, 62) KCK_B(1, 8, 55) KCK_B(2, 14, 39) KCK_B(3, 15, 41) KCK_B(4, 21, 2)
    KCK_CHI_ROW(20)
}

// Keccak-f[1600]: 24 rounds, unrolled (the round constants become literals)
GL_HD void kck_f1600(kck_state& s) {
    kck_round(s, 0x00000001u, 0x00000000u); kck_round(s, 0x00008082u, 0x00000000u); kck_round(s, 0x0000808au, 0x80000000u);
    kck_round(s, 0x80008000u, 0x80000000u); kck_round(s, 0x0000808bu, 0x00000000u); kck_round(s, 0x80000001u, 0x00000000u);
    kck_round(s, 0x80008081u, 0x80000000u); kck_round(s, 0x00008009u, 0x80000000u); kck_round(s, 0x0000008au, 0x00000000u);
    kck_round(s, 0x00000088u, 0x00000000u); kck_round(s, 0x80008009u, 0x00000000u); kck_round(s, 0x8000000au, 0x00000000u);
    kck_round(s, 0x8000808bu, 0x00000000u); kck_round(s, 0x0000008bu, 0x80000000u); kck_round(s, 0x00008089u, 0x80000000u);
    kck_round(s, 0x00008003u, 0x80000000u); kck_round(s, 0x00008002u, 0x80000000u); kck_round(s, 0x00000080u, 0x80000000u);
    kck_round(s, 0x0000800au, 0x00000000u); kck_round(s, 0x8000000au, 0x80000000u); kck_round(s, 0x80008081u, 0x80000000u);
    kck_round(s, 0x00008080u, 0x80000000u); kck_round(s, 0x80000001u, 0x00000000u); kck_round(s, 0x80008008u, 0x80000000u);
}

GL_HD void kck_clear(kck_state& s) {
#pragma unroll
    for (int i = 0; i < 25; i++) { s.lo[i] = 0; s.hi[i] = 0; }
}
// lane I ^= w, I a compile-time constant in every caller (the loops around it are unrolled)
GL_HD void kck_xor_word(kck_state& s, int i, uint64_t w) { s.lo[i] ^= (uint32_t)w; s.hi[i] ^= (uint32_t)(w >> 32); }
GL_HD uint64_t kck_word(const kck_state& s, int i) { return ((uint64_t)s.hi[i] << 32) | s.lo[i]; }
// the closing block of a message whose last block holds `rem` whole words (rem < 17): domain byte 0x01 behind them, final bit 0x80
GL_HD void kck_pad_words(kck_state& s, uint32_t rem) {
#pragma unroll
    for (int i = 0; i < KCK_RATE_WORDS; i++) if ((uint32_t)i == rem) s.lo[i] ^= 0x01u;
    s.hi[KCK_RATE_WORDS - 1] ^= 0x80000000u;
}
// the first 25 bytes of the digest as a BytesHash<25> in its four-word slot
GL_HD void kck_digest25(const kck_state& s, uint64_t out[4]) {
    out[0] = kck_word(s, 0); out[1] = kck_word(s, 1); out[2] = kck_word(s, 2); out[3] = s.lo[3] & 0xFFu;
}

#if defined(__HIPCC__)
// Absorbs the leaf whose element e is load(e) (absorbed as its canonical little-endian u64): whole 17-word blocks with compile-time
// state indices, then the tail block with the padding; `len` > 3.
template <class Load>
__device__ __forceinline__ void kck_absorb_leaf(kck_state& s, uint32_t len, Load load) {
    kck_clear(s);
    uint32_t e0 = 0;
    for (; len - e0 >= KCK_RATE_WORDS; e0 += KCK_RATE_WORDS) {
#pragma unroll
        for (int i = 0; i < KCK_RATE_WORDS; i++) kck_xor_word(s, i, gl_canon(load(e0 + i)));
        kck_f1600(s);
    }
    const uint32_t rem = len - e0;                       // 0..16 words in the closing block
#pragma unroll
    for (int i = 0; i < KCK_RATE_WORDS - 1; i++)
        if ((uint32_t)i < rem) kck_xor_word(s, i, gl_canon(load(e0 + i)));
    kck_pad_words(s, rem);
    kck_f1600(s);
}
#endif

// KeccakHash<25>::two_to_one (hash/keccak.rs:119-126): Keccak-256 of the 50 bytes left || right, one permutation.  The right digest
// starts at byte 25, so its words enter shifted by one byte.
GL_HD void kck_two_to_one(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) {
    kck_state s;
    kck_clear(s);
    kck_xor_word(s, 0, l[0]); kck_xor_word(s, 1, l[1]); kck_xor_word(s, 2, l[2]);
    kck_xor_word(s, 3, (l[3] & 0xFFu) | (r[0] << 8));
    kck_xor_word(s, 4, (r[0] >> 56) | (r[1] << 8));
    kck_xor_word(s, 5, (r[1] >> 56) | (r[2] << 8));
    kck_xor_word(s, 6, (r[2] >> 56) | ((r[3] & 0xFFu) << 8) | (uint64_t(0x01) << 16));      // bytes 48, 49, then the domain byte
    s.hi[KCK_RATE_WORDS - 1] ^= 0x80000000u;
    kck_f1600(s);
    kck_digest25(s, out);
}

// GenericHashOut::to_vec of a BytesHash<25> (hash/hash_types.rs:181-191): the bytes in chunks of 7, 7, 7, 4 as field elements -- what
// the Challenger observes and what MerkleCap::flatten puts into the circuit digest
GL_HD void kck_hash_to_elements(const uint64_t h[4], gl_t out[4]) {
    out[0] = h[0] & 0x00FFFFFFFFFFFFFFull;
    out[1] = (h[0] >> 56) | ((h[1] & 0x0000FFFFFFFFFFFFull) << 8);
    out[2] = (h[1] >> 48) | ((h[2] & 0x000000FFFFFFFFFFull) << 16);
    out[3] = (h[2] >> 40) | ((h[3] & 0xFFu) << 24);
}
GL_HD bool kck_hash_is_padded(const uint64_t h[4]) { return (h[3] >> 8) == 0; }      // the top 7 bytes of the slot are zero

// KeccakPermutation::permute's parse of the hash onion (hash/keccak.rs:84-94): the four little-endian words of one Keccak-256 output
// enter the element stream in order, words >= p are DROPPED (rejection sampling), until `want` elements are there.  `have` elements are
// in out[] already; returns the new count.  Shared by the host Challenger (want = 12) and the proof-of-work kernel (want = 8: the
// response is element 7), because the rejection branch has probability 2^-32 per word and no real hash reaches it in a test: it is
// exercised with synthetic words (tests/test_keccak.py).  The stores are a select chain so that out[] stays in registers on the device.
template <int WANT>
GL_HD uint32_t kck_words_to_elements(const uint64_t w[4], uint32_t have, gl_t (&out)[WANT]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (w[i] < GL_P && have < (uint32_t)WANT) {
#pragma unroll
            for (int k = 0; k < WANT; k++) if ((uint32_t)k == have) out[k] = w[i];
            have++;
        }
    }
    return have;
}

// Keccak-256 of the 96 bytes of a canonical 12-element sponge state: the first layer of the onion
GL_HD void kck_hash_state12(const gl_t st[12], uint64_t out[4]) {
    kck_state s;
    kck_clear(s);
#pragma unroll
    for (int i = 0; i < 12; i++) kck_xor_word(s, i, st[i]);
    s.lo[12] ^= 0x01u; s.hi[KCK_RATE_WORDS - 1] ^= 0x80000000u;
    kck_f1600(s);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = kck_word(s, i);
}
// Keccak-256 of a 32-byte digest: every further layer
GL_HD void kck_hash_32(const uint64_t in[4], uint64_t out[4]) {
    kck_state s;
    kck_clear(s);
#pragma unroll
    for (int i = 0; i < 4; i++) kck_xor_word(s, i, in[i]);
    s.lo[4] ^= 0x01u; s.hi[KCK_RATE_WORDS - 1] ^= 0x80000000u;
    kck_f1600(s);
#pragma unroll
    for (int i = 0; i < 4; i++) out[i] = kck_word(s, i);
}
// the first WANT elements of the onion H(s) || H(H(s)) || ... over the canonical state `st`
template <int WANT>
GL_HD void kck_onion(const gl_t st[12], gl_t (&out)[WANT]) {
    uint64_t h[4], g[4];
    kck_hash_state12(st, h);
    uint32_t have = kck_words_to_elements<WANT>(h, 0, out);
    while (have < (uint32_t)WANT) {
        kck_hash_32(h, g);
#pragma unroll
        for (int i = 0; i < 4; i++) h[i] = g[i];
        have = kck_words_to_elements<WANT>(h, have, out);
    }
}

// ---- host-side forms (plain loops; the device kernels of merkle.hip have their own absorb loops over column-major leaves) ----
// KeccakHash<25>::hash_no_pad (hash/keccak.rs:110-117): Keccak-256 over the elements as canonical little-endian u64, first 25 bytes
inline void kck_hash_no_pad_host(const gl_t* in, size_t n, uint64_t out[4]) {
    kck_state s;
    kck_clear(s);
    size_t off = 0;
    for (; n - off >= KCK_RATE_WORDS; off += KCK_RATE_WORDS) {
        for (int i = 0; i < KCK_RATE_WORDS; i++) kck_xor_word(s, i, gl_canon(in[off + i]));
        kck_f1600(s);
    }
    for (size_t i = 0; off + i < n; i++) kck_xor_word(s, (int)i, gl_canon(in[off + i]));
    kck_pad_words(s, (uint32_t)(n - off));
    kck_f1600(s);
    kck_digest25(s, out);
}
// Hasher::hash_or_noop (plonk/config.rs:55-66) with HASH_SIZE = 25: up to three elements are copied into the 25 bytes
inline void kck_hash_or_noop_host(const gl_t* in, size_t n, uint64_t out[4]) {
    if (n * 8 <= KCK_HASH_BYTES) { for (size_t i = 0; i < 4; i++) out[i] = i < n ? gl_canon(in[i]) : 0; return; }
    kck_hash_no_pad_host(in, n, out);
}
// KeccakPermutation::permute (hash/keccak.rs:64-95) on a 12-element sponge state
inline void kck_permute_host(gl_t state[12]) {
    gl_t c[12], out[12];
    for (int i = 0; i < 12; i++) c[i] = gl_canon(state[i]);
    kck_onion<12>(c, out);
    for (int i = 0; i < 12; i++) state[i] = out[i];
}
