// The entry points of the C ABI that never touch the GPU: the Challenger handle, the host circuit builder and witness, the gl_proof
// accessors, and the host-side hashes and keystream.  No kernels here, for context.hip's reason: this file's host pass links against
// a stub HIP runtime into a CPU harness (tools/sanitizer/abi_unwind.cpp: every allocation made to fail in turn).  The host-only object
// of a .hip file that holds a kernel cannot be linked that way.
#include "context.hpp"
#include "host_circuit.hpp"
#include "fri_instance.hpp"
#include "proof.hpp"
#include "rng.cuh"
#include <cstring>
#include <memory>

using glhost::HostChallenger;

// the Challenger handle (struct gl_challenger: fri_instance.hpp, gl_prove_openings and gl_verify_openings take it)
extern "C" gl_challenger* gl_challenger_new(void) try { return new gl_challenger(); } catch (...) { (void)gl_caught(); return nullptr; }
// Challenger::<F, H>::new (iop/challenger.rs:31-37) for H = Poseidon (0) or Keccak (1, KeccakPermutation: hash/keccak.rs:64-95)
extern "C" gl_challenger* gl_challenger_new_h(uint32_t hasher) try {
    if (hasher > GL_HASHER_KECCAK) { (void)gl_fail(GL_ERR_ARG, "gl_challenger_new_h: hasher is 0 (Poseidon) or 1 (Keccak)", __FILE__, __LINE__); return nullptr; }
    gl_challenger* c = new gl_challenger();
    c->ch.hasher = hasher;
    return c;
} catch (...) { (void)gl_caught(); return nullptr; }
// observe_hash::<OH> / observe_cap::<OH> (iop/challenger.rs:72-80; BytesHash::to_vec hash_types.rs:181-191)
extern "C" int gl_challenger_observe_hashes(gl_challenger* c, uint32_t oh, const uint64_t* h_hashes, size_t count) try {
    GL_REQUIRE(c && (h_hashes || !count) && oh <= GL_HASHER_KECCAK, GL_ERR_ARG, "gl_challenger_observe_hashes: bad argument");
    GL_REQUIRE(glhost::hashes_well_formed(oh, h_hashes, count), GL_ERR_ARG, "a BytesHash<25> slot with non-zero padding bytes");
    c->ch.observe_hashes(oh, h_hashes, count);
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" void gl_challenger_free(gl_challenger* c) noexcept { delete c; }
extern "C" int gl_challenger_observe(gl_challenger* c, const uint64_t* h_elements, size_t count) try {
    GL_REQUIRE(c && (h_elements || !count), GL_ERR_ARG, "gl_challenger_observe: null argument");
    c->ch.observe_many(h_elements, count);
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_challenger_get_challenges(gl_challenger* c, uint64_t* h_out, size_t count) try {
    GL_REQUIRE(c && (h_out || !count), GL_ERR_ARG, "gl_challenger_get_challenges: null argument");
    for (size_t i = 0; i < count; i++) h_out[i] = c->ch.challenge();
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_challenger_compact(gl_challenger* c) try {
    GL_REQUIRE(c, GL_ERR_ARG, "gl_challenger_compact: null argument");
    c->ch.compact();
    return GL_OK;
} catch (...) { return gl_caught(); }
// sponge state and pending inputs, as fri_proof_of_work reads them (fri/prover.rs:127-140): for gl_pow_grind
extern "C" int gl_challenger_state(const gl_challenger* c, uint64_t h_sponge_state[12], uint64_t h_input_buffer[8], uint32_t* input_len) try {
    GL_REQUIRE(c && h_sponge_state && h_input_buffer && input_len, GL_ERR_ARG, "gl_challenger_state: null argument");
    for (int i = 0; i < 12; i++) h_sponge_state[i] = c->ch.state[i];
    for (int i = 0; i < c->ch.nin; i++) h_input_buffer[i] = c->ch.in[i];
    *input_len = (uint32_t)c->ch.nin;
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- host circuit API ------------------------------------------------------------------------------------------------
static int matmul_circuit_build(size_t m, bool zero_knowledge, gl_host_circuit** out, uint32_t hasher = GL_HASHER_POSEIDON) {
    GL_REQUIRE(out, GL_ERR_ARG, "null out");
    GL_REQUIRE(hasher <= GL_HASHER_KECCAK, GL_ERR_ARG, "hasher is 0 (Poseidon) or 1 (Keccak)");
    std::unique_ptr<gl_host_circuit> h(new gl_host_circuit());
    int st = glhost::build_matmul(m, &h->hc, zero_knowledge, hasher);
    if (st != GL_OK) return gl_fail(st, "matmul dimension out of range (1..256)", __FILE__, __LINE__);
    *out = h.release();
    return GL_OK;
}
extern "C" int gl_matmul_circuit_build(size_t m, gl_host_circuit** out) try { return matmul_circuit_build(m, false, out); } catch (...) { return gl_caught(); }
extern "C" int gl_matmul_circuit_build_zk(size_t m, gl_host_circuit** out) try { return matmul_circuit_build(m, true, out); } catch (...) { return gl_caught(); }
// the demo's circuit under `type C = KeccakGoldilocksConfig` (plonky2/src/bin/matrix_mul.rs:21-23) or the Poseidon one, zk or not
extern "C" int gl_matmul_circuit_build_h(size_t m, uint32_t zero_knowledge, uint32_t hasher, gl_host_circuit** out) try {
    GL_REQUIRE(zero_knowledge <= 1, GL_ERR_ARG, "zero_knowledge is 0 or 1");
    return matmul_circuit_build(m, zero_knowledge != 0, out, hasher);
} catch (...) { return gl_caught(); }
extern "C" int gl_host_circuit_desc(const gl_host_circuit* hc, gl_circuit_desc* out) try {
    GL_REQUIRE(hc && out, GL_ERR_ARG, "null argument");
    *out = hc->hc.desc;
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_host_circuit_row_gates(const gl_host_circuit* hc, uint8_t* h_out) try {
    GL_REQUIRE(hc && h_out, GL_ERR_ARG, "null argument");
    memcpy(h_out, hc->hc.row_gate.data(), hc->hc.row_gate.size());
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_host_circuit_constants_sigmas(const gl_host_circuit* hc, uint64_t* h_out) try {
    GL_REQUIRE(hc && h_out, GL_ERR_ARG, "null argument");
    hc->hc.ensure_host_sigmas();
    memcpy(h_out, hc->hc.constants_sigmas.data(), hc->hc.constants_sigmas.size() * sizeof(gl_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_matmul_witness(const gl_host_circuit* hc, const uint64_t* a, const uint64_t* b, uint64_t filler_seed, uint64_t* h_wires, uint64_t* h_pis) try {
    GL_REQUIRE(hc && a && b && h_wires && h_pis, GL_ERR_ARG, "null argument");
    return glhost::matmul_witness(hc->hc, a, b, filler_seed, h_wires, h_pis);
} catch (...) { return gl_caught(); }
extern "C" void gl_host_circuit_free(gl_host_circuit* hc) noexcept { delete hc; }
extern "C" int gl_host_circuit_wire_classes(const gl_host_circuit* hc, uint64_t* h_out) try {
    GL_REQUIRE(hc && h_out, GL_ERR_ARG, "null argument");
    memcpy(h_out, hc->hc.wire_class.data(), hc->hc.wire_class.size() * sizeof(uint64_t));
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- gl_proof accessors ----------------------------------------------------------------------------------------------
extern "C" size_t gl_proof_num_bytes(const gl_proof* p) noexcept { return p ? p->bytes.size() : 0; }
extern "C" int gl_proof_bytes(const gl_proof* p, uint8_t* h_out, size_t cap) try {
    GL_REQUIRE(p && h_out && cap >= p->bytes.size(), GL_ERR_ARG, "buffer too small");
    memcpy(h_out, p->bytes.data(), p->bytes.size());
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" size_t gl_proof_challenges(const gl_proof* p, uint64_t* h_out) noexcept {
    if (!p || !h_out) return 0;
    memcpy(h_out, p->challenges.data(), p->challenges.size() * sizeof(gl_t));
    return p->challenges.size();
}
extern "C" int gl_proof_caps(const gl_proof* p, uint64_t* h_out) try {
    GL_REQUIRE(p && h_out, GL_ERR_ARG, "null argument");
    memcpy(h_out, p->caps.data(), p->caps.size() * sizeof(gl_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_proof_zs_partial_products(const gl_proof* p, uint64_t* h_out) try {
    GL_REQUIRE(p && h_out, GL_ERR_ARG, "null argument");
    GL_REQUIRE(!p->zs_pp.empty(), GL_ERR_ARG, "intermediates were not captured: call gl_ctx_capture_intermediates(ctx, 1) before proving");
    memcpy(h_out, p->zs_pp.data(), p->zs_pp.size() * sizeof(gl_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_proof_quotient_chunks(const gl_proof* p, uint64_t* h_out) try {
    GL_REQUIRE(p && h_out, GL_ERR_ARG, "null argument");
    GL_REQUIRE(!p->quotient.empty(), GL_ERR_ARG, "intermediates were not captured: call gl_ctx_capture_intermediates(ctx, 1) before proving");
    memcpy(h_out, p->quotient.data(), p->quotient.size() * sizeof(gl_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" size_t gl_proof_query_indices(const gl_proof* p, uint64_t* h_out) noexcept {
    if (!p || !h_out) return 0;
    memcpy(h_out, p->query_indices.data(), p->query_indices.size() * sizeof(uint64_t));
    return p->query_indices.size();
}
extern "C" void gl_proof_free(gl_proof* p) noexcept { delete p; }

// ---- hashes and the zero-knowledge keystream on the host -----------------------------------------------------------------
// the same two functions on the host (no GPU needed), `count` rows / pairs: hash_or_noop (plonk/config.rs:55-66) and two_to_one
// (hash/hashing.rs:98-115, hash/keccak.rs:119-126)
extern "C" int gl_hash_or_noop_host(uint32_t hasher, const uint64_t* h_rows, size_t count, size_t len, uint64_t* h_out) try {
    GL_REQUIRE_HASHER(hasher, "gl_hash_or_noop_host");
    GL_REQUIRE((h_rows || !count || !len) && (h_out || !count), GL_ERR_ARG, "gl_hash_or_noop_host: null argument");
    for (size_t r = 0; r < count; r++) glhost::hash_or_noop(hasher, h_rows + r * len, len, h_out + 4 * r);
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_two_to_one_host(uint32_t hasher, const uint64_t* h_left, const uint64_t* h_right, size_t count, uint64_t* h_out) try {
    GL_REQUIRE_HASHER(hasher, "gl_two_to_one_host");
    GL_REQUIRE((h_left && h_right && h_out) || !count, GL_ERR_ARG, "gl_two_to_one_host: null argument");
    for (size_t i = 0; i < count; i++) {
        if (hasher == GL_HASHER_KECCAK)
            GL_REQUIRE(kck_hash_is_padded(h_left + 4 * i) && kck_hash_is_padded(h_right + 4 * i), GL_ERR_ARG, "a BytesHash<25> slot with non-zero padding bytes");
        glhost::two_to_one(hasher, h_left + 4 * i, h_right + 4 * i, h_out + 4 * i);
    }
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_random_elements_host(const uint8_t seed[32], uint32_t stream, uint64_t first, uint64_t count, uint64_t* h_out) try {
    GL_REQUIRE(seed && (h_out || !count), GL_ERR_ARG, "gl_random_elements_host: null argument");
    GL_REQUIRE(first + count >= first && first + count <= (uint64_t(1) << 34), GL_ERR_ARG, "random elements: index beyond 2^34 (32-bit block counter)");
    const gl_chacha_key key = gl_chacha_key_from_bytes(seed);
    for (uint64_t i = 0; i < count; i++) h_out[i] = gl_random_element(key, stream, first + i);
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- lookups on the host ----------------------------------------------------------------------------------------------------
// permuted_cols (evm/src/lookup.rs:65-127), the reference's sequential algorithm statement by statement; gl_stark_lookup_columns
// (stark_lookup.hip) is the device form
extern "C" int gl_permuted_cols_host(const uint64_t* h_inputs, const uint64_t* h_table, size_t n, uint64_t* h_permuted_inputs, uint64_t* h_permuted_table) try {
    GL_REQUIRE(h_inputs && h_table && h_permuted_inputs && h_permuted_table && n >= 1, GL_ERR_ARG, "gl_permuted_cols_host: null argument or n == 0");
    std::vector<uint64_t> sorted_inputs(n), sorted_table(n);                           // :79-88  to_canonical, sorted by to_noncanonical_u64
    for (size_t k = 0; k < n; k++) { sorted_inputs[k] = gl_canon(h_inputs[k]); sorted_table[k] = gl_canon(h_table[k]); }
    std::sort(sorted_inputs.begin(), sorted_inputs.end());
    std::sort(sorted_table.begin(), sorted_table.end());
    std::vector<size_t> unused_table_inds;                                             // :90-92
    std::vector<uint64_t> unused_table_vals;
    unused_table_inds.reserve(n);
    unused_table_vals.reserve(n);
    std::vector<uint64_t> permuted_table(n, 0);
    size_t i = 0, j = 0;
    while (j < n && i < n) {                                                           // :95-117
        const uint64_t input_val = sorted_inputs[i], table_val = sorted_table[j];
        if (input_val > table_val) {
            unused_table_vals.push_back(sorted_table[j]);
            j++;
        } else if (input_val < table_val) {
            if (!unused_table_vals.empty()) { permuted_table[i] = unused_table_vals.back(); unused_table_vals.pop_back(); }
            else unused_table_inds.push_back(i);
            i++;
        } else {
            permuted_table[i] = sorted_table[j];
            i++;
            j++;
        }
    }
    for (; j < n; j++) unused_table_vals.push_back(sorted_table[j]);                   // :119-120
    for (; i < n; i++) unused_table_inds.push_back(i);
    GL_REQUIRE(unused_table_inds.size() == unused_table_vals.size(), GL_ERR_INTERNAL, "gl_permuted_cols_host: zip_eq of unequal lengths");      // :122
    for (size_t k = 0; k < unused_table_inds.size(); k++) permuted_table[unused_table_inds[k]] = unused_table_vals[k];
    memcpy(h_permuted_inputs, sorted_inputs.data(), n * sizeof(uint64_t));
    memcpy(h_permuted_table, permuted_table.data(), n * sizeof(uint64_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
