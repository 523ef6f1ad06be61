// The entry points of the C ABI that never touch the GPU: the Challenger handle, the host circuit builder and witness, the gl_proof
// accessors, and the host-side hashes and keystream.  No kernels here, for context.hip's reason: this file's host pass links against
// a stub HIP runtime into a CPU harness (tools/sanitizer/abi_unwind.cpp: every allocation made to fail in turn).  The host-only object
// of a .hip file that holds a kernel cannot be linked that way.
#include "context.hpp"
#include "host_circuit.hpp"
#include "fri_instance.hpp"
#include "proof.hpp"
#include "rng.cuh"
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>

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

// ---- MemoryStark on the host ------------------------------------------------------------------------------------------------
namespace {
// A polynomial over the operand words of a gl_stark_desc, as eval_packed_generic's expressions expand to: sorted factor words -> coefficient
struct MemPoly {
    std::map<std::vector<uint32_t>, int64_t> terms;
    static MemPoly constant(int64_t v) { MemPoly p; p.terms[{}] = v; return p; }
    static MemPoly operand(uint32_t kind, uint32_t col) { MemPoly p; p.terms[{kind << 30 | col}] = 1; return p; }
    MemPoly operator-(const MemPoly& o) const { MemPoly r = *this; for (const auto& t : o.terms) r.terms[t.first] -= t.second; return r; }
    MemPoly operator+(const MemPoly& o) const { MemPoly r = *this; for (const auto& t : o.terms) r.terms[t.first] += t.second; return r; }
    MemPoly operator*(const MemPoly& o) const {
        MemPoly r;
        for (const auto& a : terms)
            for (const auto& b : o.terms) {
                std::vector<uint32_t> f = a.first;
                f.insert(f.end(), b.first.begin(), b.first.end());
                std::sort(f.begin(), f.end());
                r.terms[f] += a.second * b.second;
            }
        return r;
    }
};
struct MemoryDescTables {
    std::vector<uint32_t> filter, num_terms, num_factors, factors, pair_len, pair_columns;
    std::vector<uint64_t> coeff;
    gl_stark_desc desc{};
    void yield(uint32_t filt, const MemPoly& p) {
        uint32_t k = 0;
        for (const auto& t : p.terms) {
            if (!t.second) continue;
            coeff.push_back(t.second > 0 ? (uint64_t)t.second : GL_P - (uint64_t)(-t.second));
            num_factors.push_back((uint32_t)t.first.size());
            factors.insert(factors.end(), t.first.begin(), t.first.end());
            k++;
        }
        filter.push_back(filt);
        num_terms.push_back(k);
    }
    void term(uint64_t c, std::initializer_list<uint32_t> f) { coeff.push_back(c); num_factors.push_back((uint32_t)f.size()); factors.insert(factors.end(), f.begin(), f.end()); }
    MemoryDescTables() {
        const auto local = [](uint32_t c) { return MemPoly::operand(GL_STARK_LOCAL, c); };
        const auto next = [](uint32_t c) { return MemPoly::operand(GL_STARK_NEXT, c); };
        const MemPoly one = MemPoly::constant(1);                                        // memory_stark.rs:251-264
        const MemPoly timestamp = local(GL_MEMORY_TIMESTAMP), addr_context = local(GL_MEMORY_ADDR_CONTEXT), addr_segment = local(GL_MEMORY_ADDR_SEGMENT),
                      addr_virtual = local(GL_MEMORY_ADDR_VIRTUAL);
        const MemPoly next_timestamp = next(GL_MEMORY_TIMESTAMP), next_is_read = next(GL_MEMORY_IS_READ), next_addr_context = next(GL_MEMORY_ADDR_CONTEXT),
                      next_addr_segment = next(GL_MEMORY_ADDR_SEGMENT), next_addr_virtual = next(GL_MEMORY_ADDR_VIRTUAL);
        const MemPoly filter_ = local(GL_MEMORY_FILTER);                                 // :266-274
        yield(GL_STARK_ALL, filter_ * (filter_ - one));
        const MemPoly is_dummy = one - filter_, is_write = one - local(GL_MEMORY_IS_READ);
        yield(GL_STARK_ALL, is_dummy * is_write);
        const MemPoly context_first_change = local(GL_MEMORY_CONTEXT_FIRST_CHANGE), segment_first_change = local(GL_MEMORY_SEGMENT_FIRST_CHANGE),
                      virtual_first_change = local(GL_MEMORY_VIRTUAL_FIRST_CHANGE);      // :276-287
        const MemPoly address_unchanged = one - context_first_change - segment_first_change - virtual_first_change;
        const MemPoly range_check = local(GL_MEMORY_RANGE_CHECK);
        yield(GL_STARK_ALL, context_first_change * (one - context_first_change));       // :289-293
        yield(GL_STARK_ALL, segment_first_change * (one - segment_first_change));
        yield(GL_STARK_ALL, virtual_first_change * (one - virtual_first_change));
        yield(GL_STARK_ALL, address_unchanged * (one - address_unchanged));
        yield(GL_STARK_TRANSITION, segment_first_change * (next_addr_context - addr_context));      // :295-304
        yield(GL_STARK_TRANSITION, virtual_first_change * (next_addr_context - addr_context));
        yield(GL_STARK_TRANSITION, virtual_first_change * (next_addr_segment - addr_segment));
        yield(GL_STARK_TRANSITION, address_unchanged * (next_addr_context - addr_context));
        yield(GL_STARK_TRANSITION, address_unchanged * (next_addr_segment - addr_segment));
        yield(GL_STARK_TRANSITION, address_unchanged * (next_addr_virtual - addr_virtual));
        const MemPoly computed_range_check = context_first_change * (next_addr_context - addr_context - one)      // :306-311
                                             + segment_first_change * (next_addr_segment - addr_segment - one)
                                             + virtual_first_change * (next_addr_virtual - addr_virtual - one)
                                             + address_unchanged * (next_timestamp - timestamp);
        yield(GL_STARK_TRANSITION, range_check - computed_range_check);
        for (uint32_t i = 0; i < GL_MEMORY_VALUE_LIMBS; i++)                             // :313-318
            yield(GL_STARK_TRANSITION, next_is_read * address_unchanged * (next(GL_MEMORY_VALUE_START + i) - local(GL_MEMORY_VALUE_START + i)));
        // eval_lookups (lookup.rs:13-34) on (RANGE_CHECK_PERMUTED, COUNTER_PERMUTED), term for term as api.py's lookup_constraints writes it
        const uint32_t li = GL_STARK_LOCAL << 30 | GL_MEMORY_RANGE_CHECK_PERMUTED, ni = GL_STARK_NEXT << 30 | GL_MEMORY_RANGE_CHECK_PERMUTED,
                       nt = GL_STARK_NEXT << 30 | GL_MEMORY_COUNTER_PERMUTED;
        filter.push_back(GL_STARK_ALL); num_terms.push_back(4);
        term(1, {ni, ni}); term(GL_P - 1, {ni, nt}); term(GL_P - 1, {li, ni}); term(1, {li, nt});
        filter.push_back(GL_STARK_LAST_ROW); num_terms.push_back(2);
        term(1, {ni}); term(GL_P - 1, {nt});
        pair_len = {1, 1};                                                               // :454-459
        pair_columns = {GL_MEMORY_RANGE_CHECK, GL_MEMORY_RANGE_CHECK_PERMUTED, GL_MEMORY_COUNTER, GL_MEMORY_COUNTER_PERMUTED};
        desc.num_columns = GL_MEMORY_NUM_COLUMNS; desc.num_public_inputs = 0; desc.constraint_degree = 3; desc.num_challenges = 0;
        desc.num_constraints = (uint32_t)filter.size();
        desc.constraint_filter = filter.data(); desc.constraint_num_terms = num_terms.data(); desc.term_coeff = coeff.data();
        desc.term_num_factors = num_factors.data(); desc.factors = factors.data();
        desc.num_permutation_pairs = 2; desc.pair_len = pair_len.data(); desc.pair_columns = pair_columns.data();
    }
};
}  // namespace

extern "C" int gl_memory_stark_desc(const gl_stark_desc** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_memory_stark_desc: null argument");
    static const MemoryDescTables tables;
    *out = &tables.desc;
    return GL_OK;
} catch (...) { return gl_caught(); }

// MemoryStark::generate_trace (memory_stark.rs:120-237), the reference's loops statement by statement; gl_memory_trace_fill
// (memory_trace.hip) is the device form
extern "C" int gl_memory_trace_host(const gl_memory_op* ops, size_t num_ops, uint64_t* cols_out, size_t capacity_rows, size_t* n_rows) try {
    GL_REQUIRE(ops && n_rows, GL_ERR_ARG, "gl_memory_trace_host: null argument");
    GL_REQUIRE(num_ops >= 1, GL_ERR_ARG, "gl_memory_trace_host: no memory ops");           // :195 expect("No memory ops?")
    for (size_t i = 0; i < num_ops; i++)
        GL_REQUIRE(ops[i].filter <= 1 && ops[i].is_read <= 1, GL_ERR_ARG, "gl_memory_trace_host: filter and is_read are 0 or 1");
    GL_REQUIRE(num_ops <= (size_t(1) << GL_MEMORY_MAX_LOG_ROWS), GL_ERR_UNSUPPORTED, "gl_memory_trace_host: more than 2^24 rows");
    const auto key_less = [](const gl_memory_op& a, const gl_memory_op& b) {               // MemoryOp::sorting_key, witness/memory.rs:117-124
        return std::make_tuple(a.context, a.segment, a.virt, a.timestamp) < std::make_tuple(b.context, b.segment, b.virt, b.timestamp);
    };
    const auto next_power_of_two = [](size_t k) { size_t p = 1; while (p < k) p <<= 1; return p; };
    std::vector<gl_memory_op> memory_ops(ops, ops + num_ops);
    std::stable_sort(memory_ops.begin(), memory_ops.end(), key_less);                      // :125
    const uint64_t max_rc = next_power_of_two(memory_ops.size()) - 1;                      // :164
    // what fill_gaps is about to push, counted before it pushes: one pair can ask for 2^31 rows
    uint64_t pushed = 0;
    for (size_t i = 0; i + 1 < num_ops; i++) {
        const gl_memory_op &curr = memory_ops[i], &next = memory_ops[i + 1];
        if (curr.context != next.context || curr.segment != next.segment) continue;
        if (curr.virt != next.virt) pushed += ((uint64_t)next.virt - curr.virt - 1) / (max_rc + 1);
        else if (next.timestamp != curr.timestamp) pushed += ((uint64_t)next.timestamp - curr.timestamp - 1) / max_rc;
    }
    GL_REQUIRE(num_ops + pushed <= (uint64_t(1) << GL_MEMORY_MAX_LOG_ROWS), GL_ERR_UNSUPPORTED, "gl_memory_trace_host: more than 2^24 rows");
    const std::vector<gl_memory_op> snapshot = memory_ops;                                 // :165 memory_ops.clone()
    for (size_t i = 0; i + 1 < snapshot.size(); i++) {                                     // fill_gaps, :165-191
        gl_memory_op curr = snapshot[i];
        const gl_memory_op& next = snapshot[i + 1];
        if (curr.context != next.context || curr.segment != next.segment) {
        } else if (curr.virt != next.virt) {
            while ((uint64_t)next.virt - curr.virt - 1 > max_rc) {
                gl_memory_op dummy_read{};                                                 // new_dummy_read(dummy_address, 0, U256::zero())
                dummy_read.is_read = 1;
                dummy_read.context = curr.context; dummy_read.segment = curr.segment;
                dummy_read.virt = curr.virt + (uint32_t)(max_rc + 1);
                memory_ops.push_back(dummy_read);
                curr = dummy_read;
            }
        } else {
            while ((uint64_t)next.timestamp - curr.timestamp > max_rc) {
                gl_memory_op dummy_read = curr;                                            // new_dummy_read(curr.address, curr.timestamp + max_rc, curr.value)
                dummy_read.filter = 0; dummy_read.is_read = 1;
                dummy_read.timestamp = curr.timestamp + (uint32_t)max_rc;
                memory_ops.push_back(dummy_read);
                curr = dummy_read;
            }
        }
    }
    gl_memory_op padding_op = memory_ops.back();                                           // pad_memory_ops, :194-212
    padding_op.filter = 0; padding_op.is_read = 1;
    const size_t n = next_power_of_two(memory_ops.size());
    memory_ops.resize(n, padding_op);
    std::stable_sort(memory_ops.begin(), memory_ops.end(), key_less);                      // :131
    // generate_first_change_flags_and_rc's assertion (:112-116), looked at before anything is written
    for (size_t idx = 0; idx + 1 < n; idx++) {
        const gl_memory_op &row = memory_ops[idx], &next_row = memory_ops[idx + 1];
        const uint64_t rc = row.context != next_row.context   ? (uint64_t)next_row.context - row.context - 1
                            : row.segment != next_row.segment ? (uint64_t)next_row.segment - row.segment - 1
                            : row.virt != next_row.virt       ? (uint64_t)next_row.virt - row.virt - 1
                                                              : (uint64_t)next_row.timestamp - row.timestamp;
        GL_REQUIRE(rc < n, GL_ERR_ARG, "gl_memory_trace_host: a range check is too large (a context or segment step of more than the trace's height)");
    }
    *n_rows = n;
    if (!cols_out) return GL_OK;
    GL_REQUIRE(capacity_rows >= n, GL_ERR_ARG, "gl_memory_trace_host: capacity_rows is below the trace's height");
    std::vector<uint64_t> cols((size_t)GL_MEMORY_NUM_COLUMNS * n, 0);
    const auto at = [&](uint32_t c, size_t i) -> uint64_t& { return cols[(size_t)c * n + i]; };
    for (size_t i = 0; i < n; i++) {                                                       // into_row, :52-70
        const gl_memory_op& op = memory_ops[i];
        at(GL_MEMORY_FILTER, i) = op.filter; at(GL_MEMORY_TIMESTAMP, i) = op.timestamp; at(GL_MEMORY_IS_READ, i) = op.is_read;
        at(GL_MEMORY_ADDR_CONTEXT, i) = op.context; at(GL_MEMORY_ADDR_SEGMENT, i) = op.segment; at(GL_MEMORY_ADDR_VIRTUAL, i) = op.virt;
        for (uint32_t j = 0; j < GL_MEMORY_VALUE_LIMBS; j++) at(GL_MEMORY_VALUE_START + j, i) = op.value[j];
    }
    for (size_t idx = 0; idx + 1 < n; idx++) {                                             // generate_first_change_flags_and_rc, :73-118
        const uint64_t context = at(GL_MEMORY_ADDR_CONTEXT, idx), segment = at(GL_MEMORY_ADDR_SEGMENT, idx), virt = at(GL_MEMORY_ADDR_VIRTUAL, idx),
                       timestamp = at(GL_MEMORY_TIMESTAMP, idx);
        const uint64_t next_context = at(GL_MEMORY_ADDR_CONTEXT, idx + 1), next_segment = at(GL_MEMORY_ADDR_SEGMENT, idx + 1),
                       next_virt = at(GL_MEMORY_ADDR_VIRTUAL, idx + 1), next_timestamp = at(GL_MEMORY_TIMESTAMP, idx + 1);
        const bool context_first_change = context != next_context;
        const bool segment_first_change = segment != next_segment && !context_first_change;
        const bool virtual_first_change = virt != next_virt && !segment_first_change && !context_first_change;
        at(GL_MEMORY_CONTEXT_FIRST_CHANGE, idx) = context_first_change;
        at(GL_MEMORY_SEGMENT_FIRST_CHANGE, idx) = segment_first_change;
        at(GL_MEMORY_VIRTUAL_FIRST_CHANGE, idx) = virtual_first_change;
        at(GL_MEMORY_RANGE_CHECK, idx) = context_first_change   ? next_context - context - 1
                                         : segment_first_change ? next_segment - segment - 1
                                         : virtual_first_change ? next_virt - virt - 1
                                                                : next_timestamp - timestamp;
    }
    for (size_t i = 0; i < n; i++) at(GL_MEMORY_COUNTER, i) = i;                           // generate_trace_col_major, :143-151
    GL_TRY(gl_permuted_cols_host(&at(GL_MEMORY_RANGE_CHECK, 0), &at(GL_MEMORY_COUNTER, 0), n, &at(GL_MEMORY_RANGE_CHECK_PERMUTED, 0),
                                 &at(GL_MEMORY_COUNTER_PERMUTED, 0)));
    memcpy(cols_out, cols.data(), cols.size() * sizeof(uint64_t));
    return GL_OK;
} catch (...) { return gl_caught(); }
