// Batch verify_fri_proof (fri/verifier.rs:62-241, hash/merkle_proofs.rs:54-75): the one device batch core, and the generic entry on it.
//
// What runs where.  Per proof a host stage (openings_stage.hpp: decode, challenges, proof of work, reduced openings, and whatever the
// entry checks in front of them) runs on host threads: the Challenger is a sequential sponge.  What is left is the query phase --
// num_queries x (num_oracles + num_fri_rounds) Merkle paths, independent of each other, and the field arithmetic of the queries.
// They read one record per proof, so a chunk of proofs is one upload, two launches and one download of the flags:
//   record:  T (up to the final polynomial's end) | challenge block (CH_* below) | x_index[num_queries] | caps[num_oracles][ncap][4]
//   k_verify_paths_any<HASHER>      one lane per (slot, proof, query), slot-major: leaf hash, path, comparison with the cap entry
//   k_verify_openings_queries       one lane per (proof, query): fri_combine_initial over the instance's flattened source table, per
//                                   reduction the consistency comparison and compute_evaluation, the final-polynomial Horner
// The host merges the flags in the host query loop's order, so a rejected proof reports the check gl_verify / gl_verify_openings
// reports first.  Nothing on the device trusts proof bytes: every index follows from the shape (glopen::Shape), which the decode has
// held the proof against and whose every read the core has held against the record at construction, and from x_index < 2^lgN.
// Three entries stand on the core: gl_openings_batch_verifier (below), gl_stark_batch_verifier (stark.hip, through the generic
// entry) and gl_batch_verifier (batch_verify.hip: circuit proofs).
// Not run on the device: reductions of arity above 16 (refused at construction).
#include "context.hpp"
#include "host_circuit.hpp"
#include "lanes.hpp"
#include "openings_stage.hpp"
#include "verify_lane.cuh"
#include <memory>

namespace {

using glopen::MAX_FRI_ROUNDS;
using glopen::MAX_SLOTS;

// the challenge block behind a proof's table: extension elements as word pairs; per batch b its reduced opening, alpha^len and point
enum : uint32_t { CH_ALPHA = 0, CH_BETAS = 2, CH_BATCH = CH_BETAS + 2 * MAX_FRI_ROUNDS, CH_RED = 0, CH_ALPHA_LEN = 2, CH_POINT = 4, CH_BATCH_WORDS = 6,
                  CH_WORDS = CH_BATCH + CH_BATCH_WORDS * GL_MAX_FRI_BATCHES };
constexpr uint32_t FLAG_FINAL = 1u << MAX_FRI_ROUNDS;      // k_verify_openings_queries: bit r = reduction r's consistency comparison failed

// glopen::Shape as the kernels read it (offsets in words inside one proof's record)
struct OParams {
    uint32_t num_queries, num_rounds, num_oracles, num_slots, num_batches, lgN, ncap;
    uint32_t stride;                                   // words per proof in the upload
    uint32_t o_fcaps, o_query0, query_stride, o_final, final_len, o_ch, o_x, o_caps;
    uint32_t first[GL_MAX_FRI_BATCHES + 1];
    uint32_t arity_bits[MAX_FRI_ROUNDS];
    uint32_t slot_leaf[MAX_SLOTS], slot_leaf_len[MAX_SLOTS], slot_sib[MAX_SLOTS], slot_nsib[MAX_SLOTS];
    uint32_t slot_shift[MAX_SLOTS];                    // arity bits consumed before the slot's tree: its leaf index is x_index >> shift
    gl_t w_N, w_arity[MAX_FRI_ROUNDS];                 // primitive roots of order 2^lgN and 2^arity_bits[r]
};

// ---- Merkle paths (verify_lane.cuh holds the lane body) ----
// Slot-major: the lanes of a wave share leaf length and path length (but for the one wave across a slot boundary).  An initial tree's
// cap is the claim's own, behind its table; a step tree's the commit-phase cap inside the table.
template <uint32_t HASHER>
__global__ __launch_bounds__(256) void k_verify_paths_any(const gl_t* __restrict__ in, const OParams P, uint32_t live, uint8_t* __restrict__ pass) {
    const uint32_t per_slot = live * P.num_queries, gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= per_slot * P.num_slots) return;
    const uint32_t slot = gid / per_slot, pq = gid - slot * per_slot, p = pq / P.num_queries, q = pq - p * P.num_queries;
    const gl_t* __restrict__ T = in + (size_t)p * P.stride;
    const gl_t* __restrict__ Q = T + P.o_query0 + (size_t)q * P.query_stride;
    const uint32_t idx = (uint32_t)T[P.o_x + q] >> P.slot_shift[slot];
    // idx >> nsib < 2^cap_height: the path has lg(leaves) - cap_height levels
    const gl_t* __restrict__ cap = slot < P.num_oracles ? T + P.o_caps + 4 * P.ncap * slot : T + P.o_fcaps + 4 * P.ncap * (slot - P.num_oracles);
    pass[gid] = d_path_opens_to_cap<HASHER>(Q + P.slot_leaf[slot], P.slot_leaf_len[slot], Q + P.slot_sib[slot], P.slot_nsib[slot], idx, cap) ? 1 : 0;
}

// ---- the arithmetic of one query (fri/verifier.rs:122-241) ----
typedef gl2_t E;

__global__ __launch_bounds__(64) void k_verify_openings_queries(const gl_t* __restrict__ in, const uint32_t* __restrict__ src, const OParams P, uint32_t live,
                                                                uint32_t* __restrict__ flags) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= live * P.num_queries) return;
    const uint32_t p = gid / P.num_queries, q = gid - p * P.num_queries;
    const gl_t* __restrict__ T = in + (size_t)p * P.stride;
    const gl_t* __restrict__ C = T + P.o_ch;
    const gl_t* __restrict__ Q = T + P.o_query0 + (size_t)q * P.query_stride;
    const E alpha = d_ext(C + CH_ALPHA);
    uint32_t x = (uint32_t)T[P.o_x + q];
    // subgroup_x = g * w_N^{reverse_bits(x_index)} (fri/verifier.rs:183-186)
    gl_t subgroup_x = gl_canon(gl_mul(7, gl_exp(P.w_N, __brev(x) >> (32 - P.lgN))));
    // fri_combine_initial (fri/verifier.rs:122-161): per batch Horner in alpha from its last polynomial to its first; src[j] is the
    // same for every lane (a scalar load), the leaf word is the lane's own
    const E sx = gl2_make(subgroup_x, 0);
    E eval = gl2_make(0, 0);
    for (uint32_t b = 0; b < P.num_batches; b++) {
        const gl_t* __restrict__ B = C + CH_BATCH + CH_BATCH_WORDS * b;
        E h = gl2_make(0, 0);
        for (uint32_t j = P.first[b + 1]; j-- > P.first[b];) { h = gl2_mul(h, alpha); h.a = gl_add(h.a, Q[src[j]]); }
        eval = gl2_add(gl2_mul(eval, d_ext(B + CH_ALPHA_LEN)), gl2_mul(gl2_sub(h, d_ext(B + CH_RED)), gl2_inv(gl2_sub(sx, d_ext(B + CH_POINT)))));
    }
    uint32_t bad = 0;
    for (uint32_t r = 0; r < P.num_rounds; r++) {
        const uint32_t ab = P.arity_bits[r], within = x & ((1u << ab) - 1);
        const gl_t* __restrict__ leaf = Q + P.slot_leaf[P.num_oracles + r];
        if (!d_eq(d_ext(leaf + 2 * within), eval)) bad |= 1u << r;
        eval = d_compute_evaluation(subgroup_x, within, ab, P.w_arity[r], leaf, d_ext(C + CH_BETAS + 2 * r));      // carried on whatever the comparison said, as on the host
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

using glopen::Lane;

// a refusal in the entry's own name
int refuse(int code, const glopen::Names& names, const char* what) {
    char text[256];
    snprintf(text, sizeof text, "%s_new: %s", names.entry, what);
    return gl_fail(code, text, __FILE__, __LINE__);
}

}  // namespace

struct glopen::BatchCore {
    gl_ctx* ctx = nullptr;
    Shape shape;
    Names names;
    std::string verify_name;                           // "<entry>_verify", for the lanes' failures
    OParams P;
    uint32_t max_batch = 0, host_threads = 1;
    size_t stride = 0, flag_bytes = 0;                 // words per proof in the upload; bytes of flags per proof
    gl_t *d_in = nullptr, *h_in = nullptr;
    uint32_t* d_src = nullptr;
    uint8_t *d_flags = nullptr, *h_flags = nullptr;
    std::vector<Lane> lanes;                           // one per host thread
    std::vector<uint32_t> place;                       // chunk-local proof -> its place in the upload
    std::mutex mu;                                     // calls on one core are serialised (one staging area)
};

void glopen::core_free(BatchCore* v) noexcept {
    if (!v) return;
    if (v->ctx) {
        (void)hipSetDevice(v->ctx->device);
        (void)gl_stream_wait(v->ctx->stream);
        if (v->d_in) (void)hipFree(v->d_in);
        if (v->d_src) (void)hipFree(v->d_src);
        if (v->d_flags) (void)hipFree(v->d_flags);
        if (v->h_in) (void)hipHostFree(v->h_in);
        if (v->h_flags) (void)hipHostFree(v->h_flags);
        gl_ctx_release(v->ctx);
    }
    delete v;
}

int glopen::check_batch(const Names& names, uint32_t max_batch, uint32_t host_threads) {
    if (!(max_batch >= 1 && max_batch <= 4096)) return refuse(GL_ERR_ARG, names, "max_batch is 1..4096");
    if (host_threads > GL_MAX_LANES) return refuse(GL_ERR_ARG, names, "at most 64 host threads");
    return GL_OK;
}

int glopen::core_new(gl_ctx* c, const Shape& s, uint32_t max_batch, uint32_t host_threads, const Names& names, BatchCore** out) {
    std::unique_ptr<BatchCore, void (*)(BatchCore*)> v(new BatchCore(), core_free);      // error paths free everything
    v->shape = s; v->names = names; v->verify_name = std::string(names.entry) + "_verify";
    for (uint32_t r = 0; r < s.num_rounds; r++) if (s.arity_bits[r] > 4) return refuse(GL_ERR_UNSUPPORTED, names, "a FRI arity above 16 is not supported");
    // the record: T | challenge block | x_index | caps
    const size_t cap_words = (size_t)s.num_oracles * 4 * s.ncap;
    const bool small = s.t_words <= (size_t(1) << 24);                  // (SIZE_MAX: a table that fits no size_t)
    const size_t o_ch = small ? s.t_words : 0, o_x = o_ch + CH_WORDS, o_caps = o_x + s.num_queries;
    v->stride = o_caps + cap_words;
    v->stride += v->stride & 1;
    if (!(small && v->stride <= (size_t(1) << 24) && (uint64_t)max_batch * s.num_queries * s.num_slots() < (uint64_t(1) << 31))) {
        char what[128];
        snprintf(what, sizeof what, "a proof of %s exceeds 2^24 words, or the batch 2^31 paths", names.subject);
        return refuse(GL_ERR_ARG, names, what);
    }
    v->max_batch = max_batch; v->host_threads = host_threads ? host_threads : 1;
    v->lanes.resize(v->host_threads);
    v->place.resize(max_batch);
    GL_TRY(c->activate());
    v->ctx = c; c->retain();
    if (!s.paths_fit) { *out = v.release(); return GL_OK; }      // the decode rejects every proof: nothing reaches the device, nothing is allocated
    // Nothing checks an index on the device: every read of the kernels lies inside the record, or nothing is launched
    bool inside = s.num_oracles >= 1 && s.num_oracles <= GL_MAX_FRI_ORACLES && s.num_batches <= GL_MAX_FRI_BATCHES && s.num_rounds <= MAX_FRI_ROUNDS &&
                  s.lgN >= 1 && s.lgN <= 32 && s.ncap == size_t(1) << s.cap_height && s.first[s.num_batches] == s.src.size() &&
                  s.query_stride <= (size_t(1) << 24) &&                                               // (and num_queries, by the stride)
                  s.o_fcaps + (size_t)s.num_rounds * 4 * s.ncap <= s.o_query0 && s.o_query0 + s.num_queries * s.query_stride <= s.o_final &&
                  s.o_final + 2 * s.final_len <= s.t_words && o_caps + cap_words <= v->stride;
    for (uint32_t j : s.src) inside = inside && j < s.query_stride;
    unsigned lg_cur = s.lgN;
    for (uint32_t slot = 0; slot < s.num_slots() && inside; slot++) {
        if (slot >= s.num_oracles) lg_cur -= s.arity_bits[slot - s.num_oracles];
        inside = s.slot_leaf[slot] + s.slot_leaf_len[slot] <= s.query_stride && s.slot_sib[slot] + 4 * s.slot_nsib[slot] <= s.query_stride &&
                 s.slot_nsib[slot] + s.cap_height == lg_cur &&                                         // the cap entry idx >> nsib exists
                 (slot < s.num_oracles || (s.arity_bits[slot - s.num_oracles] >= 1 && s.slot_leaf_len[slot] == size_t(2) << s.arity_bits[slot - s.num_oracles]));
    }
    if (!inside) return refuse(GL_ERR_INTERNAL, names, "the shape's reads leave its record");
    v->flag_bytes = (size_t)s.num_queries * (sizeof(uint32_t) + s.num_slots());
    OParams& P = v->P;
    P = OParams();
    P.num_queries = s.num_queries; P.num_rounds = s.num_rounds; P.num_oracles = s.num_oracles; P.num_slots = s.num_slots(); P.num_batches = s.num_batches;
    P.lgN = s.lgN; P.ncap = (uint32_t)s.ncap; P.stride = (uint32_t)v->stride;
    P.o_fcaps = (uint32_t)s.o_fcaps; P.o_query0 = (uint32_t)s.o_query0; P.query_stride = (uint32_t)s.query_stride; P.o_final = (uint32_t)s.o_final;
    P.final_len = (uint32_t)s.final_len; P.o_ch = (uint32_t)o_ch; P.o_x = (uint32_t)o_x; P.o_caps = (uint32_t)o_caps;
    for (uint32_t b = 0; b <= GL_MAX_FRI_BATCHES; b++) P.first[b] = s.first[b];
    uint32_t consumed = 0;
    for (uint32_t slot = 0; slot < s.num_slots(); slot++) {
        if (slot >= s.num_oracles) {
            const uint32_t r = slot - s.num_oracles;
            P.arity_bits[r] = s.arity_bits[r]; P.w_arity[r] = glhost::root_of_unity(s.arity_bits[r]);
            consumed += s.arity_bits[r];
        }
        P.slot_leaf[slot] = (uint32_t)s.slot_leaf[slot]; P.slot_leaf_len[slot] = (uint32_t)s.slot_leaf_len[slot];
        P.slot_sib[slot] = (uint32_t)s.slot_sib[slot]; P.slot_nsib[slot] = (uint32_t)s.slot_nsib[slot]; P.slot_shift[slot] = consumed;
    }
    P.w_N = glhost::root_of_unity(s.lgN);
    GL_CHECK_HIP(hipMalloc((void**)&v->d_in, v->stride * sizeof(gl_t) * max_batch));
    GL_CHECK_HIP(hipHostMalloc((void**)&v->h_in, v->stride * sizeof(gl_t) * max_batch, hipHostMallocDefault));
    GL_CHECK_HIP(hipMalloc((void**)&v->d_flags, v->flag_bytes * max_batch));
    GL_CHECK_HIP(hipHostMalloc((void**)&v->h_flags, v->flag_bytes * max_batch, hipHostMallocDefault));
    GL_CHECK_HIP(hipMalloc((void**)&v->d_src, s.src.size() * sizeof(uint32_t)));
    GL_CHECK_HIP(hipMemcpyAsync(v->d_src, s.src.data(), s.src.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    GL_CHECK_HIP(gl_stream_wait(c->stream));
    *out = v.release();
    return GL_OK;
}

// one chunk of at most max_batch proofs: host stage on the lanes, then upload, two launches, download and the merge
static int verify_chunk(glopen::BatchCore* v, size_t first, size_t count, const glopen::Stage& stage, int32_t* verdicts, uint32_t* checks) {
    const glopen::Shape& s = v->shape;
    constexpr uint32_t REJECTED = UINT32_MAX;
    const size_t cap_words = (size_t)s.num_oracles * 4 * s.ncap;
    std::atomic<uint32_t> live{0};
    GL_TRY(gl_run_lanes(v->host_threads, count, v->verify_name.c_str(), [&](size_t lane, size_t i) {
        v->place[i] = REJECTED;
        Lane& L = v->lanes[lane];
        L.caps = nullptr; L.verdict = GL_OK; L.check = GL_CHECK_ACCEPTED;
        GL_TRY(stage(lane, first + i, L));
        verdicts[i] = L.verdict;
        if (checks) checks[i] = L.check;
        if (L.verdict == GL_OK) {
            GL_REQUIRE(v->h_in && L.caps && L.T.size() >= s.t_words && L.ch.x_index.size() == s.num_queries, GL_ERR_INTERNAL, "batch verification: a stage passed a proof it did not fill");
            const uint32_t at = live.fetch_add(1, std::memory_order_relaxed);
            v->place[i] = at;
            gl_t* dst = v->h_in + (size_t)at * v->stride;
            memcpy(dst, L.T.data(), s.t_words * sizeof(gl_t));
            gl_t* C = dst + v->P.o_ch;
            auto put = [&](uint32_t where, gl2_t e) { e = gl2_canon(e); C[where] = e.a; C[where + 1] = e.b; };
            put(CH_ALPHA, L.ch.alpha);
            for (uint32_t r = 0; r < MAX_FRI_ROUNDS; r++) put(CH_BETAS + 2 * r, L.ch.betas[r]);
            for (uint32_t b = 0; b < GL_MAX_FRI_BATCHES; b++) {
                const uint32_t at_b = CH_BATCH + CH_BATCH_WORDS * b;
                put(at_b + CH_RED, L.ch.red[b]); put(at_b + CH_ALPHA_LEN, L.ch.alpha_len[b]); put(at_b + CH_POINT, L.ch.point[b]);
            }
            for (uint32_t q = 0; q < s.num_queries; q++) dst[v->P.o_x + q] = L.ch.x_index[q];
            // the caps as path_opens_to_cap compares them: a HashOut's words as field elements, a BytesHash<25>'s as they are
            for (size_t k = 0; k < cap_words; k++) dst[v->P.o_caps + k] = s.hasher == GL_HASHER_KECCAK ? L.caps[k] : gl_canon(L.caps[k]);
        }
        return GL_OK;
    }));
    const uint32_t n = live.load();
    if (!n) return GL_OK;
    GL_REQUIRE(v->d_in, GL_ERR_INTERNAL, "batch verification: a proof passed the decode of a description no proof fits");
    gl_ctx* c = v->ctx;
    GL_TRY(c->activate());
    const uint32_t nq = s.num_queries, slots = s.num_slots(), per_slot = n * nq;
    uint32_t* d_fri = reinterpret_cast<uint32_t*>(v->d_flags);
    uint8_t* d_pass = v->d_flags + sizeof(uint32_t) * per_slot;
    {
        GlTimed t(c, v->names.scope);
        GL_CHECK_HIP(hipMemcpyAsync(v->d_in, v->h_in, (size_t)n * v->stride * sizeof(gl_t), hipMemcpyHostToDevice, c->stream));
        if (s.hasher == GL_HASHER_KECCAK)
            hipLaunchKernelGGL(k_verify_paths_any<GL_HASHER_KECCAK>, dim3((per_slot * slots + 255) / 256), dim3(256), 0, c->stream, v->d_in, v->P, n, d_pass);
        else
            hipLaunchKernelGGL(k_verify_paths_any<GL_HASHER_POSEIDON>, dim3((per_slot * slots + 255) / 256), dim3(256), 0, c->stream, v->d_in, v->P, n, d_pass);
        GL_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_verify_openings_queries, dim3((per_slot + 63) / 64), dim3(64), 0, c->stream, v->d_in, v->d_src, v->P, n, d_fri);
        GL_CHECK_HIP(hipGetLastError());
        GL_CHECK_HIP(hipMemcpyAsync(v->h_flags, v->d_flags, v->flag_bytes * n, hipMemcpyDeviceToHost, c->stream));
    }
    GL_CHECK_HIP(gl_stream_wait(c->stream));
    // The host loop's order: queries ascending; within one the initial trees in order, per reduction the consistency comparison
    // before the step tree's Merkle proof, then the final polynomial.  The device evaluates every query of a proof and the host stops
    // at the first failure; only the first failure is reported, so the first failing flag in this order is the host's check.
    const uint32_t* fri = reinterpret_cast<const uint32_t*>(v->h_flags);
    const uint8_t* pass = v->h_flags + sizeof(uint32_t) * per_slot;
    for (size_t i = 0; i < count; i++) {
        if (v->place[i] == REJECTED) continue;
        const uint32_t base = v->place[i] * nq;
        uint32_t check = GL_CHECK_ACCEPTED;
        for (uint32_t q = 0; q < nq && !check; q++) {
            const uint32_t f = fri[base + q];
            for (uint32_t o = 0; o < s.num_oracles && !check; o++) if (!pass[o * per_slot + base + q]) check = GL_CHECK_INITIAL_MERKLE;
            for (uint32_t r = 0; r < s.num_rounds && !check; r++) {
                if ((f >> r) & 1) check = GL_CHECK_FRI_CONSISTENCY;
                else if (!pass[(s.num_oracles + r) * per_slot + base + q]) check = GL_CHECK_STEP_MERKLE;
            }
            if (!check && (f & FLAG_FINAL)) check = GL_CHECK_FINAL_POLY;
        }
        if (check) { verdicts[i] = GL_ERR_VERIFY; if (checks) checks[i] = check; }
    }
    return GL_OK;
}

int glopen::core_verify(BatchCore* v, size_t count, const Stage& stage, int32_t* verdicts, uint32_t* checks) {
    std::lock_guard<std::mutex> lk(v->mu);
    for (size_t at = 0; at < count; at += v->max_batch) {
        const size_t k = count - at < v->max_batch ? count - at : v->max_batch;
        GL_TRY(verify_chunk(v, at, k, stage, verdicts + at, checks ? checks + at : nullptr));
    }
    return GL_OK;
}

// ---- the generic entry: glfri::check in front of the core, glopen::host_stage as its stage ----
struct gl_openings_batch_verifier {
    gl_fri_params params;
    gl_fri_instance instance;                          // polys points into `polys`
    std::vector<uint32_t> polys;
    glopen::Shape shape;
    glopen::BatchCore* core = nullptr;
};

extern "C" void gl_openings_batch_verifier_free(gl_openings_batch_verifier* v) noexcept {
    if (!v) return;
    glopen::core_free(v->core);
    delete v;
}

int glopen::batch_new(gl_ctx* c, const gl_fri_params* params, const gl_fri_instance* instance, uint32_t max_batch, uint32_t host_threads,
                      gl_openings_batch_verifier** out) {
    const Names names = {"gl_openings_batch_verifier", "these params", "openings_batch_verify"};
    GL_REQUIRE(c, GL_ERR_ARG, "gl_openings_batch_verifier_new: null argument");
    GL_TRY(check_batch(names, max_batch, host_threads));
    std::unique_ptr<gl_openings_batch_verifier, void (*)(gl_openings_batch_verifier*)> v(new gl_openings_batch_verifier(), gl_openings_batch_verifier_free);
    GL_REQUIRE(params && instance, GL_ERR_ARG, "FRI openings: null params / instance");
    // the instance without its points: every claim brings its own (an opening point off the base field passes the coset check)
    v->params = *params; v->instance = *instance;
    for (uint32_t b = 0; b < GL_MAX_FRI_BATCHES; b++) { v->instance.points[b][0] = 0; v->instance.points[b][1] = 1; }
    GL_TRY(shape_of(&v->params, &v->instance, v->shape));
    const Shape& s = v->shape;
    v->polys.assign(instance->polys, instance->polys + 2 * s.src.size());
    v->instance.polys = v->polys.data();
    GL_TRY(core_new(c, s, max_batch, host_threads, names, &v->core));
    *out = v.release();
    return GL_OK;
}

extern "C" int gl_openings_batch_verifier_new(gl_ctx* c, const gl_fri_params* params, const gl_fri_instance* instance, uint32_t max_batch, uint32_t host_threads,
                                              gl_openings_batch_verifier** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_openings_batch_verifier_new: null argument");
    *out = nullptr;
    GL_REQUIRE(c && params && instance, GL_ERR_ARG, "gl_openings_batch_verifier_new: null argument");
    return glopen::batch_new(c, params, instance, max_batch, host_threads, out);
} catch (...) { return gl_caught(); }

int glopen::batch_verify(gl_openings_batch_verifier* v, size_t count, const ClaimSource& source, int32_t* verdicts, uint32_t* checks) {
    return core_verify(v->core, count, [&](size_t lane, size_t i, Lane& L) -> int {
        gl_openings_claim claim = {};
        const int st = source(lane, i, claim, &L.check);
        if (st == GL_ERR_VERIFY) { L.verdict = st; return GL_OK; }
        if (st != GL_OK) return st;
        L.caps = claim.caps;
        return L.judged(host_stage(v->params, v->instance, v->shape, claim.points, claim.caps, claim.openings, claim.challenger, claim.proof, claim.num_bytes, L.T, L.ch, &L.check));
    }, verdicts, checks);
}

extern "C" int gl_openings_batch_verifier_verify(gl_openings_batch_verifier* v, const gl_openings_claim* claims, size_t count, int32_t* verdicts,
                                                 uint32_t* checks) try {
    GL_REQUIRE(v, GL_ERR_ARG, "gl_openings_batch_verifier_verify: null verifier");
    if (!count) return GL_OK;
    GL_REQUIRE(claims && verdicts, GL_ERR_ARG, "gl_openings_batch_verifier_verify: null argument");
    return glopen::batch_verify(v, count, [&](size_t, size_t i, gl_openings_claim& claim, uint32_t*) -> int {
        claim = claims[i];
        GL_REQUIRE(claim.caps && claim.openings && claim.points && claim.challenger && claim.proof, GL_ERR_ARG, "gl_openings_batch_verifier_verify: null argument in a claim");
        return GL_OK;
    }, verdicts, checks);
} catch (...) { return gl_caught(); }
