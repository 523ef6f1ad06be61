// Batch verification: VerifierCircuitData::verify for many proofs of one circuit (plonk/verifier.rs:15-115, fri/verifier.rs:62-260,
// hash/merkle_proofs.rs:54-75).
//
// What runs where.  Per proof the host stage of gl_verify (verify_stage.hpp: decode, transcript, vanishing identity at zeta, proof of
// work) runs on host threads: its sponges are sequential (the public-input hash, the Challenger), so a proof gives a device lane nothing
// to do side by side.  What is left are the hashes of the query phase -- 28 queries x (4 initial + num_fri_rounds step) Merkle paths,
// independent of each other -- and the field arithmetic of the queries.  They read only the decoded word table T of the proof and a small
// challenge block, so a chunk of proofs is one upload, two launches and one download of the pass flags:
//   k_verify_merkle_paths<HASHER>   one lane per (slot, proof, query): leaf hash, path, comparison with the cap entry
//   k_verify_fri_queries            one lane per (proof, query): fri_combine_initial, per round the consistency comparison and
//                                   compute_evaluation, the final-polynomial Horner
// The host merges the flags in gl_verify's order, so a rejected proof reports the check gl_verify reports first.
// Nothing on the device trusts proof bytes: every index follows from the description (glverify::Shape), which the decode has held the
// proof against, and from x_index < 2^lgN.
#include "context.hpp"
#include "host_circuit.hpp"
#include "lanes.hpp"
#include "verify_lane.cuh"
#include "verify_stage.hpp"
#include <memory>

namespace {

using glverify::CHALLENGE_WORDS;
using glverify::MAX_FRI_ROUNDS;
using glverify::MAX_SLOTS;
using glverify::NUM_INITIAL_TREES;

// the challenge block behind a proof's table: extension elements as word pairs, then the query indices
enum : uint32_t { CH_ZETA = 0, CH_GZETA = 2, CH_ALPHA = 4, CH_BETAS = 6, CH_RED0 = 6 + 2 * MAX_FRI_ROUNDS, CH_RED1 = CH_RED0 + 2, CH_SHIFT = CH_RED1 + 2, CH_X = CH_SHIFT + 2 };
static_assert(CH_X == CHALLENGE_WORDS, "the challenge block and its size are one fact");
constexpr uint32_t FLAG_FINAL = 1u << MAX_FRI_ROUNDS;      // k_verify_fri_queries: bit r = round r's consistency comparison failed

// glverify::Shape as the kernels read it (offsets in words inside one proof's table; slot s < 4: initial tree s, 4 + r: step tree r)
struct VParams {
    uint32_t num_queries, num_rounds, num_slots, lgN, ncap, nzp;
    uint32_t stride, t_words;                          // words per proof in the upload: the table, then the challenge block
    uint32_t o_caps, o_fcaps, o_query0, query_stride, o_final, final_len;
    uint32_t widths[4];
    uint32_t arity_bits[MAX_FRI_ROUNDS];
    uint32_t slot_leaf[MAX_SLOTS], slot_leaf_len[MAX_SLOTS], slot_sib[MAX_SLOTS], slot_nsib[MAX_SLOTS];
    uint32_t slot_shift[MAX_SLOTS];                    // arity bits consumed before the slot's tree: its leaf index is x_index >> shift
    gl_t w_N, w_arity[MAX_FRI_ROUNDS];                 // primitive roots of order 2^lgN and 2^arity_bits[r]
};

// ---- Merkle paths (hash/merkle_proofs.rs:54-75; leaf hash plonk/config.rs:55-66) ----
// The grid is slot-major: the lanes of a wave share leaf length and path length (but for the one wave across a slot boundary), so
// they run the same number of permutations.  Poseidon through psd_permute, the VALU layer: it holds under any EXEC mask, and the
// launch is a few thousand lanes, far from filling the matrix cores.
template <uint32_t HASHER>
__global__ __launch_bounds__(256) void k_verify_merkle_paths(const gl_t* __restrict__ in, const gl_t* __restrict__ cap0, const VParams P, uint32_t live,
                                                             uint8_t* __restrict__ pass) {
    const uint32_t per_slot = live * P.num_queries, gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= per_slot * P.num_slots) return;
    const uint32_t slot = gid / per_slot, pq = gid - slot * per_slot, p = pq / P.num_queries, q = pq - p * P.num_queries;
    const gl_t* __restrict__ T = in + (size_t)p * P.stride;
    const gl_t* __restrict__ Q = T + P.o_query0 + (size_t)q * P.query_stride;
    const gl_t* __restrict__ leaf = Q + P.slot_leaf[slot];
    const gl_t* __restrict__ sib = Q + P.slot_sib[slot];
    const uint32_t len = P.slot_leaf_len[slot], nsib = P.slot_nsib[slot];
    const uint32_t idx = (uint32_t)T[P.t_words + CH_X + q] >> P.slot_shift[slot];
    // idx >> nsib < 2^cap_height: the path has lg(leaves) - cap_height levels
    const gl_t* __restrict__ cap = slot == 0 ? cap0 : slot < NUM_INITIAL_TREES ? T + P.o_caps + 4 * P.ncap * (slot - 1) : T + P.o_fcaps + 4 * P.ncap * (slot - NUM_INITIAL_TREES);
    pass[gid] = d_path_opens_to_cap<HASHER>(leaf, len, sib, nsib, idx, cap) ? 1 : 0;
}

// ---- the arithmetic of one query (fri/verifier.rs:124-241) ----
typedef gl2_t E;
// acc = acc * alpha + v[i] for i = last - 1 down to first (base-field values)
__device__ __forceinline__ E d_horner_base(E acc, E alpha, const gl_t* __restrict__ v, uint32_t first, uint32_t last) {
    for (uint32_t i = last; i-- > first;) { acc = gl2_mul(acc, alpha); acc.a = gl_add(acc.a, v[i]); }
    return acc;
}

__global__ __launch_bounds__(64) void k_verify_fri_queries(const gl_t* __restrict__ in, const VParams P, uint32_t live, uint32_t* __restrict__ flags) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= live * P.num_queries) return;
    const uint32_t p = gid / P.num_queries, q = gid - p * P.num_queries;
    const gl_t* __restrict__ T = in + (size_t)p * P.stride;
    const gl_t* __restrict__ C = T + P.t_words;
    const gl_t* __restrict__ Q = T + P.o_query0 + (size_t)q * P.query_stride;
    const E zeta = d_ext(C + CH_ZETA), gzeta = d_ext(C + CH_GZETA), alpha = d_ext(C + CH_ALPHA);
    uint32_t x = (uint32_t)C[CH_X + q];
    // subgroup_x = g * w_N^{reverse_bits(x_index)} (fri/verifier.rs:183-186)
    gl_t subgroup_x = gl_canon(gl_mul(7, gl_exp(P.w_N, __brev(x) >> (32 - P.lgN))));
    // fri_combine_initial (fri/verifier.rs:124-165): Horner in alpha over the unsalted prefixes, from the last polynomial of a batch to
    // its first; batch 0 = constants_sigmas, wires, Z and partial products, quotient, lookups; batch 1 = Z, lookups
    const gl_t* __restrict__ leaf2 = Q + P.slot_leaf[2];
    E h0 = d_horner_base(gl2_make(0, 0), alpha, leaf2, P.nzp, P.widths[2]);
    h0 = d_horner_base(h0, alpha, Q + P.slot_leaf[3], 0, P.widths[3]);
    h0 = d_horner_base(h0, alpha, leaf2, 0, P.nzp);
    h0 = d_horner_base(h0, alpha, Q + P.slot_leaf[1], 0, P.widths[1]);
    h0 = d_horner_base(h0, alpha, Q + P.slot_leaf[0], 0, P.widths[0]);
    E h1 = d_horner_base(gl2_make(0, 0), alpha, leaf2, P.nzp, P.widths[2]);
    h1 = d_horner_base(h1, alpha, leaf2, 0, 2);
    const E sx = gl2_make(subgroup_x, 0);
    E eval = gl2_mul(gl2_sub(h0, d_ext(C + CH_RED0)), gl2_inv(gl2_sub(sx, zeta)));
    eval = gl2_add(gl2_mul(eval, d_ext(C + CH_SHIFT)), gl2_mul(gl2_sub(h1, d_ext(C + CH_RED1)), gl2_inv(gl2_sub(sx, gzeta))));
    uint32_t bad = 0;
    for (uint32_t r = 0; r < P.num_rounds; r++) {
        const uint32_t ab = P.arity_bits[r], arity = 1u << ab, within = x & (arity - 1);
        const gl_t* __restrict__ leaf = Q + P.slot_leaf[NUM_INITIAL_TREES + r];
        if (!d_eq(d_ext(leaf + 2 * within), eval)) bad |= 1u << r;
        eval = d_compute_evaluation(subgroup_x, within, ab, P.w_arity[r], leaf, d_ext(C + CH_BETAS + 2 * r));      // the host carries its own value on as well (and stops at the first failure)
        for (uint32_t i = 0; i < ab; i++) subgroup_x = gl_sqr(subgroup_x);
        x >>= ab;
    }
    E fin = gl2_make(0, 0);
    const E sxf = gl2_make(gl_canon(subgroup_x), 0);
    const gl_t* __restrict__ fp = T + P.o_final;
    for (uint32_t i = P.final_len; i-- > 0;) fin = gl2_add(gl2_mul(fin, sxf), d_ext(fp + 2 * i));
    if (!d_eq(fin, eval)) bad |= FLAG_FINAL;
    flags[gid] = bad;
}

struct Lane { std::vector<gl_t> T; glverify::Challenges ch; };

}  // namespace

struct gl_batch_verifier {
    gl_ctx* ctx = nullptr;
    gl_circuit_desc desc;
    glverify::Shape shape;
    VParams params;
    std::vector<uint64_t> cap;                         // as the caller gave it (the host stage reads it)
    uint64_t digest[4];
    uint32_t max_batch = 0, host_threads = 1;
    size_t stride = 0, flag_bytes = 0;                 // words per proof in the upload; bytes of flags per proof
    gl_t *d_in = nullptr, *h_in = nullptr, *d_cap = nullptr;
    uint8_t *d_flags = nullptr, *h_flags = nullptr;
    std::vector<Lane> lanes;                           // one per host thread
    std::vector<uint32_t> place;                       // chunk-local proof -> its place in the upload
    std::mutex mu;                                     // calls on one verifier are serialised (one staging area)
};

extern "C" void gl_batch_verifier_free(gl_batch_verifier* v) noexcept {
    if (!v) return;
    if (v->ctx) {
        (void)hipSetDevice(v->ctx->device);
        (void)gl_stream_wait(v->ctx->stream);
        if (v->d_in) (void)hipFree(v->d_in);
        if (v->d_cap) (void)hipFree(v->d_cap);
        if (v->d_flags) (void)hipFree(v->d_flags);
        if (v->h_in) (void)hipHostFree(v->h_in);
        if (v->h_flags) (void)hipHostFree(v->h_flags);
        gl_ctx_release(v->ctx);
    }
    delete v;
}

extern "C" int gl_batch_verifier_new(gl_ctx* c, const gl_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                                     uint32_t max_batch, uint32_t host_threads, gl_batch_verifier** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_batch_verifier_new: null argument");
    *out = nullptr;
    GL_REQUIRE(c && desc && constants_sigmas_cap && circuit_digest, GL_ERR_ARG, "gl_batch_verifier_new: null argument");
    GL_REQUIRE(max_batch >= 1 && max_batch <= 4096, GL_ERR_ARG, "gl_batch_verifier_new: max_batch is 1..4096");
    GL_REQUIRE(host_threads <= GL_MAX_LANES, GL_ERR_ARG, "gl_batch_verifier_new: at most 64 host threads");
    std::unique_ptr<gl_batch_verifier, void (*)(gl_batch_verifier*)> v(new gl_batch_verifier(), gl_batch_verifier_free);      // error paths free everything
    GL_TRY(glverify::shape_of(*desc, SIZE_MAX, v->shape));
    const glverify::Shape& s = v->shape;
    for (uint32_t r = 0; r < s.num_rounds; r++) GL_REQUIRE(s.arity_bits[r] <= 4, GL_ERR_UNSUPPORTED, "gl_batch_verifier_new: a FRI arity above 16 is not supported");
    GL_REQUIRE(s.t_words <= (size_t(1) << 24) && (uint64_t)max_batch * s.num_queries * s.num_slots() < (uint64_t(1) << 31), GL_ERR_ARG,
               "gl_batch_verifier_new: a proof of this description exceeds 2^24 words, or the batch 2^31 paths");
    v->desc = *desc;
    v->cap.assign(constants_sigmas_cap, constants_sigmas_cap + 4 * s.ncap);
    for (int k = 0; k < 4; k++) v->digest[k] = circuit_digest[k];
    v->max_batch = max_batch; v->host_threads = host_threads ? host_threads : 1;
    v->lanes.resize(v->host_threads);
    v->place.resize(max_batch);
    v->stride = s.t_words + CHALLENGE_WORDS + s.num_queries;
    v->stride += v->stride & 1;
    v->flag_bytes = (size_t)s.num_queries * (sizeof(uint32_t) + s.num_slots());
    VParams& P = v->params;
    P = VParams();
    P.num_queries = s.num_queries; P.num_rounds = s.num_rounds; P.num_slots = s.num_slots(); P.lgN = s.lgN; P.ncap = (uint32_t)s.ncap; P.nzp = (uint32_t)s.nzp;
    P.stride = (uint32_t)v->stride; P.t_words = (uint32_t)s.t_words;
    P.o_caps = (uint32_t)s.o_caps; P.o_fcaps = (uint32_t)s.o_fcaps; P.o_query0 = (uint32_t)s.o_query0; P.query_stride = (uint32_t)s.query_stride;
    P.o_final = (uint32_t)s.o_final; P.final_len = (uint32_t)s.final_len;
    for (int o = 0; o < 4; o++) P.widths[o] = (uint32_t)s.widths[o];
    uint32_t consumed = 0;
    for (uint32_t slot = 0; slot < s.num_slots() && s.paths_fit; slot++) {
        if (slot >= NUM_INITIAL_TREES) {
            const uint32_t r = slot - NUM_INITIAL_TREES;
            P.arity_bits[r] = s.arity_bits[r]; P.w_arity[r] = glhost::root_of_unity(s.arity_bits[r]);
            consumed += s.arity_bits[r];
        }
        P.slot_leaf[slot] = (uint32_t)s.slot_leaf[slot]; P.slot_leaf_len[slot] = (uint32_t)s.slot_leaf_len[slot];
        P.slot_sib[slot] = (uint32_t)s.slot_sib[slot]; P.slot_nsib[slot] = (uint32_t)s.slot_nsib[slot]; P.slot_shift[slot] = consumed;
    }
    P.w_N = glhost::root_of_unity(s.lgN);
    GL_TRY(c->activate());
    v->ctx = c; c->retain();
    if (s.paths_fit) {                                 // (otherwise gl_verify rejects every proof in the decode: nothing reaches the device)
        GL_CHECK_HIP(hipMalloc((void**)&v->d_in, v->stride * sizeof(gl_t) * max_batch));
        GL_CHECK_HIP(hipHostMalloc((void**)&v->h_in, v->stride * sizeof(gl_t) * max_batch, hipHostMallocDefault));
        GL_CHECK_HIP(hipMalloc((void**)&v->d_flags, v->flag_bytes * max_batch));
        GL_CHECK_HIP(hipHostMalloc((void**)&v->h_flags, v->flag_bytes * max_batch, hipHostMallocDefault));
        GL_CHECK_HIP(hipMalloc((void**)&v->d_cap, 4 * s.ncap * sizeof(gl_t)));
        // the cap as path_opens_to_cap compares it: a HashOut's words as field elements, a BytesHash<25>'s as they are
        for (size_t i = 0; i < 4 * s.ncap; i++) v->h_in[i] = s.hasher == GL_HASHER_KECCAK ? v->cap[i] : gl_canon(v->cap[i]);
        GL_CHECK_HIP(hipMemcpyAsync(v->d_cap, v->h_in, 4 * s.ncap * sizeof(gl_t), hipMemcpyHostToDevice, c->stream));
        GL_CHECK_HIP(gl_stream_wait(c->stream));
    }
    *out = v.release();
    return GL_OK;
} catch (...) { return gl_caught(); }

// one chunk of at most max_batch proofs: host stage on the lanes, then upload, two launches, download and the merge
static int verify_chunk(gl_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count, int32_t* verdicts, uint32_t* checks) {
    const glverify::Shape& s = v->shape;
    const gl_circuit_desc& d = v->desc;
    constexpr uint32_t REJECTED = UINT32_MAX;
    std::atomic<uint32_t> live{0};
    GL_TRY(gl_run_lanes(v->host_threads, count, "gl_batch_verifier_verify", [&](size_t lane, size_t i) {
        v->place[i] = REJECTED;
        GL_REQUIRE(proofs[i], GL_ERR_ARG, "gl_batch_verifier_verify: null proof");
        if (!(d.num_query_rounds <= num_bytes[i] / 8 && d.num_public_inputs <= num_bytes[i] / 8)) {      // gl_verify's one check of the description against the proof
            verdicts[i] = GL_ERR_ARG;
            if (checks) checks[i] = GL_CHECK_DESCRIPTION;
            return GL_OK;
        }
        Lane& L = v->lanes[lane];
        uint32_t check = GL_CHECK_ACCEPTED;
        const int st = glverify::host_stage(d, s, v->cap.data(), v->digest, proofs[i], num_bytes[i], L.T, L.ch, &check);
        if (st != GL_OK && st != GL_ERR_VERIFY) return st;
        verdicts[i] = st;
        if (checks) checks[i] = check;
        if (st == GL_OK) {
            const uint32_t at = live.fetch_add(1, std::memory_order_relaxed);
            v->place[i] = at;
            gl_t* dst = v->h_in + (size_t)at * v->stride;
            memcpy(dst, L.T.data(), s.t_words * sizeof(gl_t));
            gl_t* C = dst + s.t_words;
            auto put = [&](uint32_t where, gl2_t e) { e = gl2_canon(e); C[where] = e.a; C[where + 1] = e.b; };
            put(CH_ZETA, L.ch.zeta); put(CH_GZETA, L.ch.gzeta); put(CH_ALPHA, L.ch.fri_alpha);
            for (uint32_t r = 0; r < MAX_FRI_ROUNDS; r++) put(CH_BETAS + 2 * r, L.ch.fri_betas[r]);
            put(CH_RED0, L.ch.red0); put(CH_RED1, L.ch.red1); put(CH_SHIFT, L.ch.alpha_shift);
            for (uint32_t q = 0; q < s.num_queries; q++) C[CH_X + q] = L.ch.x_index[q];
        }
        return GL_OK;
    }));
    const uint32_t n = live.load();
    if (!n) return GL_OK;
    GL_REQUIRE(v->d_in, GL_ERR_INTERNAL, "gl_batch_verifier_verify: a proof passed the decode of a description no proof fits");
    gl_ctx* c = v->ctx;
    GL_TRY(c->activate());
    const uint32_t nq = s.num_queries, slots = s.num_slots(), per_slot = n * nq;
    uint32_t* d_fri = reinterpret_cast<uint32_t*>(v->d_flags);
    uint8_t* d_pass = v->d_flags + sizeof(uint32_t) * per_slot;
    {
        GlTimed t(c, "batch_verify");
        GL_CHECK_HIP(hipMemcpyAsync(v->d_in, v->h_in, (size_t)n * v->stride * sizeof(gl_t), hipMemcpyHostToDevice, c->stream));
        if (s.hasher == GL_HASHER_KECCAK)
            hipLaunchKernelGGL(k_verify_merkle_paths<GL_HASHER_KECCAK>, dim3((per_slot * slots + 255) / 256), dim3(256), 0, c->stream, v->d_in, v->d_cap, v->params, n, d_pass);
        else
            hipLaunchKernelGGL(k_verify_merkle_paths<GL_HASHER_POSEIDON>, dim3((per_slot * slots + 255) / 256), dim3(256), 0, c->stream, v->d_in, v->d_cap, v->params, n, d_pass);
        GL_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_verify_fri_queries, dim3((per_slot + 63) / 64), dim3(64), 0, c->stream, v->d_in, v->params, n, d_fri);
        GL_CHECK_HIP(hipGetLastError());
        GL_CHECK_HIP(hipMemcpyAsync(v->h_flags, v->d_flags, v->flag_bytes * n, hipMemcpyDeviceToHost, c->stream));
    }
    GL_CHECK_HIP(gl_stream_wait(c->stream));
    // gl_verify's order: queries ascending; within one the initial trees 0..3, per round the consistency comparison before the step
    // tree's Merkle proof, then the final polynomial.  The first failing flag is the proof's check.
    const uint32_t* fri = reinterpret_cast<const uint32_t*>(v->h_flags);
    const uint8_t* pass = v->h_flags + sizeof(uint32_t) * per_slot;
    for (size_t i = 0; i < count; i++) {
        if (v->place[i] == REJECTED) continue;
        const uint32_t base = v->place[i] * nq;
        uint32_t check = GL_CHECK_ACCEPTED;
        for (uint32_t q = 0; q < nq && !check; q++) {
            const uint32_t f = fri[base + q];
            for (uint32_t o = 0; o < NUM_INITIAL_TREES && !check; o++) if (!pass[o * per_slot + base + q]) check = GL_CHECK_INITIAL_MERKLE;
            for (uint32_t r = 0; r < s.num_rounds && !check; r++) {
                if ((f >> r) & 1) check = GL_CHECK_FRI_CONSISTENCY;
                else if (!pass[(NUM_INITIAL_TREES + r) * per_slot + base + q]) check = GL_CHECK_STEP_MERKLE;
            }
            if (!check && (f & FLAG_FINAL)) check = GL_CHECK_FINAL_POLY;
        }
        if (check) { verdicts[i] = GL_ERR_VERIFY; if (checks) checks[i] = check; }
    }
    return GL_OK;
}

extern "C" int gl_batch_verifier_verify(gl_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count, int32_t* verdicts,
                                        uint32_t* checks) try {
    GL_REQUIRE(v, GL_ERR_ARG, "gl_batch_verifier_verify: null verifier");
    if (!count) return GL_OK;
    GL_REQUIRE(proofs && num_bytes && verdicts, GL_ERR_ARG, "gl_batch_verifier_verify: null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    for (size_t at = 0; at < count; at += v->max_batch) {
        const size_t k = count - at < v->max_batch ? count - at : v->max_batch;
        GL_TRY(verify_chunk(v, proofs + at, num_bytes + at, k, verdicts + at, checks ? checks + at : nullptr));
    }
    return GL_OK;
} catch (...) { return gl_caught(); }
