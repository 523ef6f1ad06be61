// The randomness of zero-knowledge proving (the reference draws it from thread_rng: RandomValueGenerator, iop/generator.rs;
// PolynomialBatch salts, fri/oracle.rs:100-125): a keyed counter-based generator that the device kernels and the host share.
//
//   keystream  ChaCha20 block function of RFC 8439 section 2.3: key = the 32-byte seed, nonce = (stream as u32 LE, 0, 0),
//              block counter = block index from 0
//   element i  (w_{2i} + 2^64 w_{2i+1}) mod p over the keystream's little-endian u64 words w_k: 4 elements per block,
//              canonical, within 2^-64 of uniform
//   streams    0x100 + w: blinding value of wire column w, element index = row
//              0x200 + 4 o + j: salt column j (0..3) of PlonkOracle o (1 wires, 2 zs_partial_products, 3 quotient),
//              element index = natural LDE row
//
// Plain 32-bit adds, xors and rotates on both sides; every array index is a compile-time constant after unrolling, so the
// state lives in registers.
#pragma once
#include <stdint.h>
#include "gl64.cuh"

enum : uint32_t { GL_STREAM_WIRE = 0x100, GL_STREAM_SALT = 0x200 };
enum { GL_SALT_SIZE = 4 };      // fri/oracle.rs:26

struct gl_chacha_key { uint32_t w[8]; };

GL_HD uint32_t gl_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define GL_CHACHA_QR(a, b, c, d)                    \
    a += b; d ^= a; d = gl_rotl32(d, 16);           \
    c += d; b ^= c; b = gl_rotl32(b, 12);           \
    a += b; d ^= a; d = gl_rotl32(d, 8);            \
    c += d; b ^= c; b = gl_rotl32(b, 7);

// RFC 8439 section 2.3: the 16 output words of block `counter` of stream `stream` (nonce = stream, 0, 0)
GL_HD void gl_chacha20_block(const gl_chacha_key& k, uint32_t stream, uint32_t counter, uint32_t out[16]) {
    uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
    uint32_t x4 = k.w[0], x5 = k.w[1], x6 = k.w[2], x7 = k.w[3], x8 = k.w[4], x9 = k.w[5], x10 = k.w[6], x11 = k.w[7];
    uint32_t x12 = counter, x13 = stream, x14 = 0, x15 = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        GL_CHACHA_QR(x0, x4, x8, x12) GL_CHACHA_QR(x1, x5, x9, x13) GL_CHACHA_QR(x2, x6, x10, x14) GL_CHACHA_QR(x3, x7, x11, x15)
        GL_CHACHA_QR(x0, x5, x10, x15) GL_CHACHA_QR(x1, x6, x11, x12) GL_CHACHA_QR(x2, x7, x8, x13) GL_CHACHA_QR(x3, x4, x9, x14)
    }
    out[0] = x0 + 0x61707865u; out[1] = x1 + 0x3320646eu; out[2] = x2 + 0x79622d32u; out[3] = x3 + 0x6b206574u;
    out[4] = x4 + k.w[0]; out[5] = x5 + k.w[1]; out[6] = x6 + k.w[2]; out[7] = x7 + k.w[3];
    out[8] = x8 + k.w[4]; out[9] = x9 + k.w[5]; out[10] = x10 + k.w[6]; out[11] = x11 + k.w[7];
    out[12] = x12 + counter; out[13] = x13 + stream; out[14] = x14; out[15] = x15;
}
#undef GL_CHACHA_QR

// element j (0..3) of a block: (w_{2j} + 2^64 w_{2j+1}) mod p
GL_HD gl_t gl_chacha_element(const uint32_t out[16], uint32_t j) {
    uint32_t a = 0, b = 0, c = 0, d = 0;
#pragma unroll
    for (uint32_t t = 0; t < 4; t++)
        if (t == j) { a = out[4 * t]; b = out[4 * t + 1]; c = out[4 * t + 2]; d = out[4 * t + 3]; }
    return gl_canon(gl_reduce128((uint64_t)a | ((uint64_t)b << 32), (uint64_t)c | ((uint64_t)d << 32)));
}
GL_HD gl_t gl_random_element(const gl_chacha_key& k, uint32_t stream, uint64_t index) {
    uint32_t out[16];
    gl_chacha20_block(k, stream, (uint32_t)(index >> 2), out);
    return gl_chacha_element(out, (uint32_t)(index & 3));
}

inline gl_chacha_key gl_chacha_key_from_bytes(const uint8_t seed[32]) {
    gl_chacha_key k;
    for (int i = 0; i < 8; i++)
        k.w[i] = (uint32_t)seed[4 * i] | ((uint32_t)seed[4 * i + 1] << 8) | ((uint32_t)seed[4 * i + 2] << 16) | ((uint32_t)seed[4 * i + 3] << 24);
    return k;
}
