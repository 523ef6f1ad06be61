// Library context: one per (device, stream).  Owns twiddle / power tables and scratch memory so that
// no entry point allocates or synchronises on its hot path (graph-capture friendly after warm-up).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <chrono>
#include <time.h>
#include <sys/prctl.h>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <map>
#include <new>
#include <tuple>
#include <mutex>
#include <unordered_map>
#include <string>
#include <utility>
#include <vector>
#include "gl64.cuh"
#include "../../include/plonky2_mi355x.h"

struct gl_ctx;
void gl_ctx_release(gl_ctx* c);      // drops one reference (context.hip)

// ---- errors: the C ABI never unwinds ----------------------------------------------------------------------
// The calling thread's last error text.  A fixed buffer, so that reporting an error allocates nothing: the path that
// reports "out of host memory" must not need any.  `what` must not point into the buffer itself.
inline thread_local char g_gl_last_error[512] = "";
inline int gl_fail(int code, const char* what, const char* file, int line) noexcept {
    snprintf(g_gl_last_error, sizeof g_gl_last_error, "%s (%s:%d)", what, file, line);
    return code;
}
// The one exception boundary.  Every extern "C" definition whose body can throw is a function-try-block
//     extern "C" int gl_foo(...) try { body } catch (...) { return gl_caught(); }
// (a pointer return: `(void)gl_caught(); return nullptr;`); the ones whose body cannot throw -- the *_free functions
// and plain getters -- are declared noexcept instead.  tests/test_abi.py checks that every definition is one or the other.
inline int gl_caught() noexcept {
    try { throw; }
    catch (const std::bad_alloc&) { return gl_fail(GL_ERR_INTERNAL, "out of host memory", __FILE__, __LINE__); }
    catch (const std::exception& e) { return gl_fail(GL_ERR_INTERNAL, e.what(), __FILE__, __LINE__); }
    catch (...) { return gl_fail(GL_ERR_INTERNAL, "unknown C++ exception", __FILE__, __LINE__); }
}

#define GL_CHECK_HIP(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return gl_fail(GL_ERR_HIP, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define GL_REQUIRE(cond, code, msg)                                      \
    do {                                                                 \
        if (!(cond)) return gl_fail(code, msg, __FILE__, __LINE__);      \
    } while (0)
#define GL_REQUIRE_HASHER(h, who) GL_REQUIRE((h) == GL_HASHER_POSEIDON || (h) == GL_HASHER_KECCAK, GL_ERR_ARG, who ": hasher is 0 (Poseidon) or 1 (Keccak)")
#define GL_TRY(expr)                 \
    do {                             \
        int _s = (expr);             \
        if (_s != GL_OK) return _s;  \
    } while (0)

// Wait for a stream by polling it.  hipStreamSynchronize follows the device's scheduling flags, and a process that has brought
// up RCCL blocks on an interrupt there: every one of the ~10 transcript round trips of a proof then pays a wake-up latency
// (measured: 245 -> 210 proofs/s with a one-rank process group).  Polling is independent of what other libraries set.
// One or two waiting threads spin (a lone proof's latency is the sum of ~15 such waits, and a sleeping poll adds ~35 us to
// each: 6.3 -> 6.8 ms measured).  With more waiters -- many proofs in flight -- a wait lasts milliseconds, and spinning threads
// exhaust the CPU quota (measured on the 1-GPU box, 16 lanes: the cgroup throttled the process in half of its scheduling
// periods, and 24 or 32 lanes ran 20-40 % SLOWER than 16) and keep threads that have work to submit off the cores when several
// ranks share a host: after ~50 us those threads sleep ~20 us between polls.
inline std::atomic<int> gl_stream_waiters{0};
// proofs currently inside gl_prove* in this process (any context): with several in flight the GPU's issue slots are the bound
// and latency-hiding variants that spend more instructions per result stop paying (merkle.hip gl_coop_max_nodes)
inline std::atomic<int> gl_proofs_in_flight{0};
inline hipError_t gl_stream_wait(hipStream_t s) {
    hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return e;
    static thread_local bool slack_set = false;
    struct Count { Count() { gl_stream_waiters.fetch_add(1, std::memory_order_relaxed); } ~Count() { gl_stream_waiters.fetch_sub(1, std::memory_order_relaxed); } } count;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (gl_stream_waiters.load(std::memory_order_relaxed) <= 2 || std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(50)) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        } else {
            // (the first sleeping wait of a thread lowers ITS timer slack from the default 50 us to 1 us; nothing else is changed)
            if (!slack_set) { (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0); slack_set = true; }
            struct timespec ts = {0, 20000};
            (void)nanosleep(&ts, nullptr);
        }
    }
}

// ---- wave priority of the small, dependent launches ---------------------------------------------------------
// A launch of at most one wave per SIMD lasts as long as one wave's dependent chain, and with 16 proofs in flight that wave
// lands beside the long-lived waves of the bulk kernels (a leaf-hash wave lives for 17 permutations).  VALU issue between
// co-resident waves goes by priority, then age: at equal priority the newcomer gets the leftover slots, its launch lasts
// several times its lone duration, and the hardware queue behind it -- shared by other proofs -- waits.  Such a launch is
// *urgent*: its kernel raises its waves' priority as its first statement, gl_raise_prio(prio), prio being a kernel argument
// (or a field of the params struct) and so wave-uniform: s_setprio ignores EXEC.  The instruction count does not change; the
// bulk waves give up the issue slots the small launch needs anyway.
// Only for kernels that never spin on memory: a raised wave that polls starves the wave it waits for.
#ifndef GL_URGENT_PRIO
#define GL_URGENT_PRIO 1                        // the one raised tier (priority 1 already outranks every other wave, all at 0)
#endif
// two waves per SIMD (256 CUs x 4): with 16 proofs in flight 2048 gave 339.2 proofs/s against 336.4 for 1024 and 320.1 for 0
// with the tree levels and tops alone, 343.0 against 339.9 with the FRI / permutation chain and the NTT passes as well
// (m = 64: the first level of a 2^18-leaf tree is 2048 waves).  The leaf-hash kernels are NOT guarded: with the leaf launches
// of the small trees raised as well the rate fell back to 327 (profiles/urgent_prio_ab.txt) -- presumably because a leaf wave,
// older and longer-lived, then outranks the level wave beside it again.
#define GL_URGENT_MAX_WAVES_DEFAULT 2048u
// tuning knob (environment GL_URGENT_MAX_WAVES): launches of at most this many waves are urgent; 0 = never
inline uint32_t gl_urgent_max_waves() {
    static const uint32_t v = [] { const char* e = getenv("GL_URGENT_MAX_WAVES"); return e ? (uint32_t)strtoul(e, nullptr, 10) : GL_URGENT_MAX_WAVES_DEFAULT; }();
    return v;
}
// the priority argument of a launch of `total_threads` threads: 0, or GL_URGENT_PRIO when the launch is urgent
inline int gl_launch_prio(uint64_t total_threads) { return (total_threads + 63) / 64 <= gl_urgent_max_waves() ? GL_URGENT_PRIO : 0; }
// (the instruction takes its level as an immediate)
__device__ __forceinline__ void gl_raise_prio(int prio) { if (prio) __builtin_amdgcn_s_setprio(GL_URGENT_PRIO); }

static const gl_t GL_MULT_GENERATOR = 7;                          // field/src/goldilocks_field.rs:80
static const gl_t GL_POW2_GENERATOR = 1753635133440165772ULL;     // field/src/goldilocks_field.rs:87

inline gl_t gl_host_root_of_unity(unsigned lg) {                   // field/src/types.rs:268-272
    gl_t r = GL_POW2_GENERATOR;
    for (unsigned i = lg; i < 32; i++) r = gl_sqr(r);
    return gl_canon(r);
}
inline gl_t gl_host_inverse_2exp(unsigned e) { return GL_P - ((GL_P - 1) >> e); }   // types.rs:227-266

struct GlPowTable {
    gl_t* lo = nullptr;   // base^j, j < 2048
    gl_t* hi = nullptr;   // scale * base^(2048 j)
    uint32_t hi_len = 0;
};

struct gl_ctx {
    // Lifetime: one reference for the creator (dropped by gl_ctx_destroy) plus one per live handle that points at this context
    // (gl_batch, gl_merkle, gl_circuit, gl_fri, gl_matmul_witgen).  The context -- its stream, tables and allocator -- is torn
    // down when the last reference goes, so handles may be freed after gl_ctx_destroy in any order.
    std::atomic<int> refs{1};
    void retain() { refs.fetch_add(1, std::memory_order_relaxed); }
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool own_queue = false;                                       // the stream has a hardware queue of its own (context.hip "lane queues")
    gl_t* tw_local[2] = {nullptr, nullptr};                       // w_4096^e forward / inverse
    std::map<std::pair<gl_t, gl_t>, GlPowTable> pow_tables;       // (base, scale) -> table
    std::map<std::tuple<gl_t, gl_t, uint32_t>, gl_t*> pass_tables; // (w_N, scale, lgN1) -> scale * inter-pass twiddles in column-pass output order
    int get_pass_table(gl_t w, gl_t scale, uint32_t lgN1, uint32_t lgN2, const gl_t** out);
    gl_t* scratch = nullptr;
    size_t scratch_elems = 0;
    // inter-pass scratch: at most 2^26 elements (512 MiB), i.e. 64 polynomials of 2^20 per column/row launch pair.  Fewer, larger
    // launches beat keeping the scratch Infinity-Cache resident: forward 2^20 x 64 takes 0.829 / 0.751 / 0.737 / 0.722 ms with
    // 2^23 / 2^24 / 2^25 / 2^26 elements (8 / 4 / 2 / 1 launch pairs); prove() is indifferent (+0.6 %)
    size_t scratch_target = size_t(1) << 26;
    // pinned staging buffers for small device-to-host results (caps, openings, query rows).  A context's stream may be used by
    // several host threads at once (proofs on other contexts read the shared circuit's batches through ITS context), so a
    // buffer is taken from this list for one copy and handed back afterwards
    std::mutex pin_mu;
    std::vector<std::pair<void*, size_t>> pin_free;
    size_t pin_count = 0;                                         // buffers that exist, free or in use (pin_free has room for all of them)
    int pin_acquire(size_t bytes, void** out, size_t* cap);
    void pin_release(void* p, size_t cap) noexcept;
    gl_t* dev_small = nullptr;                                    // 1 MiB device staging
    size_t dev_small_bytes = 0;

    // optional per-launch timing (HIP events on the ctx stream); scope names follow the reference's
    // TimingTree labels where one exists (plonky2/src/util/timing.rs, fri/oracle.rs:51-89)
    struct TimingRec { const char* name; hipEvent_t start, stop; };
    bool timing_enabled = false;
    std::vector<TimingRec> timing_recs;
    std::vector<size_t> timing_stack;       // open scopes (scopes nest like the reference's TimingTree)
    void timing_begin(const char* name);
    void timing_end();

    // Stream-ordered caching allocator: prove() allocates the same buffer sizes for every proof, and hipMalloc /
    // hipFree synchronise the whole device (which would serialise proofs running on other streams).  Blocks are
    // recycled within this context only; all work of a context is ordered on its one stream, so a block may be
    // handed out again without waiting for the kernels that last used it.
    std::mutex pool_mu;
    std::multimap<size_t, void*> pool_free_blocks;
    std::unordered_map<void*, size_t> pool_block_size;
    size_t pool_bytes = 0;
    int pool_alloc(size_t bytes, void** out);
    void pool_release(void* p) noexcept;      // (destructors and *_free call it)
    void pool_trim() noexcept;

    // parity tests: keep the Z / partial-product values and the quotient chunks of each proof on the host
    bool capture_intermediates = false;

    int activate();
    int ensure_scratch(size_t elems);
    int ensure_dev_small(size_t bytes);
    int get_pow_table(gl_t base, gl_t scale, uint32_t hi_len, GlPowTable* out);
    std::vector<gl_t*> retired_tables;      // superseded (shorter) power tables: possibly still in flight, freed with the context
    // small read-only index tables (Merkle leaf element offsets, ...) cached by content
    std::map<std::vector<uint64_t>, uint64_t*> offset_tables;
    int get_offsets_table(const uint64_t* host, size_t len, const uint64_t** d_out);
};

// RAII scope of the optional per-launch timing
struct GlTimed {
    gl_ctx* c;
    GlTimed(gl_ctx* ctx, const char* name) : c(ctx) { c->timing_begin(name); }
    ~GlTimed() { c->timing_end(); }
};

// ---- NTT launcher (ntt.hip) ---------------------------------------------------------------------------
int gl_ntt_local_tables(gl_ctx* c);      // fills c->tw_local on c->stream: the part of gl_ctx_create that needs kernels
// dst[b][k] = post_const * post_shift^k * sum_i (pre_shift^i * src[b][i]) * w^(+-ik),  i < n_in, k < 2^lgN
// pre_shift / post_shift == 0 mean "no scaling".  src may equal dst.  Output canonical.
int gl_ntt_run(gl_ctx* ctx, const gl_t* src, uint64_t src_stride, uint32_t n_in, gl_t* dst, uint64_t dst_stride,
               uint32_t lgN, uint32_t batch, bool inverse, gl_t pre_shift, gl_t post_shift, gl_t post_const);

// ---- Merkle (merkle.hip) ------------------------------------------------------------------------------
struct GlMerkle {
    uint32_t lg_leaves = 0, cap_height = 0, leaf_len = 0;
    uint32_t hasher = 0;                     // 0 Poseidon (HashOut digests), 1 Keccak (BytesHash<25> in the same four-word slots)
    gl_t* digests = nullptr;                 // levels concatenated, level l at level_off[l] (in digests)
    std::vector<uint64_t> level_off;         // in units of digests (4 x u64)
    uint64_t total_digests = 0;
    gl_t* level_ptr(uint32_t l) const { return digests + 4 * level_off[l]; }
    uint32_t num_levels() const { return lg_leaves - cap_height + 1; }
};
// leaf r (natural order) has elements base[offsets[e] + r], e < leaf_len; it is leaf bitrev(r) of the tree
int gl_merkle_build(gl_ctx* ctx, const gl_t* base, const uint64_t* host_offsets, uint32_t leaf_len,
                    uint32_t lg_leaves, uint32_t cap_height, GlMerkle* out, uint32_t hasher = 0);
void gl_merkle_release(gl_ctx* ctx, GlMerkle* m);
int gl_merkle_prove_impl(gl_ctx* c, const GlMerkle& m, size_t leaf_index, uint64_t* h_out, uint32_t* n_siblings);

// ---- PolynomialBatch (batch.hip) ------------------------------------------------------------------------
struct gl_batch {
    gl_ctx* ctx = nullptr;
    size_t ncols = 0, n = 0;
    uint32_t degree_log = 0, rate_bits = 0, cap_height = 0;
    uint32_t hasher = 0;         // C::Hasher of the Merkle tree: 0 Poseidon, 1 Keccak
    uint32_t salt = 0;           // 0, or GL_SALT_SIZE random columns behind the LDE (blinding, fri/oracle.rs:100-125)
    gl_t* coeffs = nullptr;      // [ncols][n]
    gl_t* lde = nullptr;         // [ncols + salt][N], natural order (index i <-> 7 * w_N^i); the salt columns only enter the leaves
    GlMerkle tree;
    size_t N() const { return n << rate_bits; }
    size_t leaf_len() const { return ncols + salt; }
};
// from_values / from_coeffs of a device matrix with the salt columns of PlonkOracle `oracle` drawn from `seed` (rng.cuh); a null seed
// commits without salt, as gl_batch_from_device
int gl_batch_from_device_salted(gl_ctx* c, const uint64_t* d_cols, size_t ncols, size_t n, uint32_t rate_bits, uint32_t cap_height,
                                int is_values, const uint8_t* seed, uint32_t oracle, gl_batch** out, uint32_t hasher = 0);

// ---- randomness (rng.hip) -------------------------------------------------------------------------------
// 32 bytes from getrandom(2)
int gl_os_seed(uint8_t seed[32]);
// d_out[s * out_stride + i] = element first + i of stream stream0 + s (rng.cuh), s < nstreams, i < count
int gl_fill_random(gl_ctx* c, const uint8_t seed[32], uint32_t stream0, uint32_t nstreams, uint64_t first, uint64_t count, gl_t* d_out,
                   uint64_t out_stride);
// the blinding rows of a zero-knowledge witness d_wires[135][n] from row g on (circuit_builder.rs:777-818 + full_witness)
int gl_launch_witness_blind(gl_ctx* c, const uint8_t seed[32], gl_t* d_wires, uint32_t n, uint32_t g, uint32_t regular, uint32_t pairs);

// RAII block from a context's stream-ordered pool
struct DevBuf {
    gl_ctx* c; void* p = nullptr;
    explicit DevBuf(gl_ctx* ctx) : c(ctx) {}
    int alloc(size_t bytes) { return c->pool_alloc(bytes, &p); }
    void release() { if (p) { c->pool_release(p); p = nullptr; } }
    ~DevBuf() { release(); }
    template <class T> T* as() const { return (T*)p; }
};
