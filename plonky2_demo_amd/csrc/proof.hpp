// The proof handle of the C ABI: prove.hip fills it, host_api.hip reads it back out; and the byte writers every proof writer shares
// (prove.hip: circuit proofs and the FriProof of gl_prove_openings; stark.hip: STARK proofs).
#pragma once
#include <stdint.h>
#include <vector>
#include "gl64.cuh"
#include "../../include/plonky2_mi355x.h"

struct gl_proof {
    std::vector<uint8_t> bytes;
    std::vector<gl_t> challenges;     // betas gammas alphas zeta fri_alpha pow pi_hash fri_betas...
    std::vector<gl_t> caps;           // 3 x 16 x 4
    std::vector<gl_t> zs_pp;          // [20][n]
    std::vector<gl_t> quotient;       // [16][n]
    std::vector<uint64_t> query_indices;
};

// ---- little-endian proof bytes (util/serialization/mod.rs): one definition, so the writers cannot drift apart ----
inline void put_u64(std::vector<uint8_t>& o, uint64_t v) { for (int i = 0; i < 8; i++) o.push_back((uint8_t)(v >> (8 * i))); }
inline void put_words(std::vector<uint8_t>& o, const gl_t* v, size_t n) { for (size_t i = 0; i < n; i++) put_u64(o, gl_canon(v[i])); }
// write_hash (util/serialization/mod.rs:248-256): a HashOut is four field elements, a BytesHash<25> its 25 bytes
inline size_t hash_wire_bytes(uint32_t hasher) { return hasher == GL_HASHER_KECCAK ? 25 : 32; }
inline void put_hashes(std::vector<uint8_t>& o, uint32_t hasher, const gl_t* h, size_t count) {
    if (hasher != GL_HASHER_KECCAK) { put_words(o, h, 4 * count); return; }
    for (size_t i = 0; i < count; i++) {
        for (int k = 0; k < 3; k++) put_u64(o, h[4 * i + k]);
        o.push_back((uint8_t)h[4 * i + 3]);
    }
}
// owns a batch for the length of a scope
struct BatchHolder { gl_batch* b = nullptr; ~BatchHolder() { if (b) gl_batch_free(b); } };
