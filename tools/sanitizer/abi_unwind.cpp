// Host-only AddressSanitizer / UBSan harness for the promise of include/plonky2_mi355x.h that no entry point unwinds: global
// operator new is replaced by one that throws std::bad_alloc at the k-th allocation of the calling thread, and every listed call
// is run once clean (A allocations), then once per k < A with allocation k failing, then clean again.  A failing run must come back
// as a GL_ERR_* status (or a null handle) with a text in gl_last_error() and its out-handles null; the last clean run must give the
// first one's result, so no state was damaged on the way; LeakSanitizer sees whatever an unwinding path dropped.  CPU only: the host
// passes of host_api.hip, verifier.hip, serialization.hip and context.hip over the stub runtime of hip_stub.cpp, and the lane runner
// (lanes.hpp).  argv[1] = directory with desc.bin, cap.bin, dig.bin, proof.bin, vd.bin of the m = 2 matmul circuit
// (tests/test_abi_unwind.py).  Exit code 0 = every line below says "A allocations, A failed cleanly".
#include "../../plonky2_demo_amd/csrc/lanes.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

// ---- the injector ----------------------------------------------------------------------------------------------------
static thread_local long t_count = 0, t_fail_at = -1;
static void* counted_alloc(size_t n) {
    if (t_count++ == t_fail_at) return nullptr;
    return malloc(n ? n : 1);
}
void* operator new(size_t n) { if (void* p = counted_alloc(n)) return p; throw std::bad_alloc(); }
void* operator new[](size_t n) { if (void* p = counted_alloc(n)) return p; throw std::bad_alloc(); }
void* operator new(size_t n, const std::nothrow_t&) noexcept { return counted_alloc(n); }
void* operator new[](size_t n, const std::nothrow_t&) noexcept { return counted_alloc(n); }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }
void operator delete(void* p, const std::nothrow_t&) noexcept { free(p); }
void operator delete[](void* p, const std::nothrow_t&) noexcept { free(p); }

static int g_bad = 0;
static void bad(const char* name, long k, const char* what) { printf("%s: allocation %ld: %s\n", name, k, what); g_bad++; }
static uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}

// One listed call.  prepare() and cleanup() run without injection; call() makes the library call(s) and nothing else that allocates,
// and returns the status; outputs_null() says whether a failed call left its out-handles null; result() is what a clean run computed.
// With `retry`, every failed call is followed by a clean one on the SAME handles, which must give the first run's result: a handle
// that went through a failed call stays usable.
template <class Prepare, class Call, class Null, class Result, class Cleanup>
static void sweep(const char* name, Prepare prepare, Call call, Null outputs_null, Result result, Cleanup cleanup, bool retry = false) {
    auto run = [&](long fail_at, long* allocations) {
        g_gl_last_error[0] = 0;
        t_count = 0; t_fail_at = fail_at;
        const int st = call();
        t_fail_at = -1;
        if (allocations) *allocations = t_count;
        return st;
    };
    long A = 0, clean = 0;
    prepare();
    const int st0 = run(-1, &A);
    const uint64_t r0 = st0 == GL_OK ? result() : 0;
    cleanup();
    if (st0 != GL_OK) { bad(name, -1, "the clean run failed"); printf("  %s\n", gl_last_error()); return; }
    for (long k = 0; k < A; k++) {
        prepare();
        const int st = run(k, nullptr);
        if (st == GL_OK) bad(name, k, "the call succeeded");
        else if (!gl_last_error()[0]) bad(name, k, "no text in gl_last_error()");
        else if (!outputs_null()) bad(name, k, "an out-handle is not null");
        else if (retry && (run(-1, nullptr) != GL_OK || result() != r0)) bad(name, k, "the same call on the same handle afterwards differs from the first run");
        else clean++;
        cleanup();
    }
    prepare();
    const int st1 = run(-1, nullptr);
    if (st1 != GL_OK || result() != r0) bad(name, A, "the clean run after the failures differs from the first");
    cleanup();
    printf("%s: %ld allocations, %ld failed cleanly\n", name, A, clean);
}
static bool yes() { return true; }
static void nothing() {}

static std::vector<unsigned char> rd(const std::string& p) {
    FILE* f = fopen(p.c_str(), "rb"); std::vector<unsigned char> v; if (!f) return v;
    int c; while ((c = fgetc(f)) != EOF) v.push_back((unsigned char)c);
    fclose(f); return v;
}

static gl_ctx* make_ctx() {                 // over the stub runtime: no device, and no twiddle tables (hip_stub.cpp)
    gl_ctx* c = nullptr;
    if (gl_ctx_create(0, nullptr, &c) != GL_OK) abort();
    return c;
}

// ---- the lane runner: 4 lanes, 10 items --------------------------------------------------------------------------------
static void lane_cases() {
    int done[10];
    auto reset = [&] { for (int& d : done) d = 0; };
    auto count = [&] { int n = 0; for (int d : done) n += d; return n; };
    // a lane that throws on its first item.  What the other lanes finish before the failure is recorded is up to the scheduler, so
    // only this is required: the status, the text, none of the failing lane's own items done, the rest at most all done
    for (size_t lane : {size_t(0), size_t(2)}) {
        reset();
        const int st = gl_run_lanes(4, 10, "abi_unwind", [&](size_t l, size_t i) -> int { if (l == lane) throw std::bad_alloc(); done[i] = 1; return GL_OK; });
        bool own = false;
        for (size_t i = lane; i < 10; i += 4) own = own || done[i];
        if (st != GL_ERR_INTERNAL || !strstr(gl_last_error(), "out of host memory") || own || count() > (lane == 0 ? 7 : 8))
            bad("lanes: std::bad_alloc in a lane", (long)lane, gl_last_error());
    }
    printf("lanes: std::bad_alloc thrown on lane 0 and on lane 2 became GL_ERR_INTERNAL\n");
    reset();
    int st = gl_run_lanes(4, 10, "abi_unwind", [&](size_t, size_t i) -> int { if (i == 5) throw std::runtime_error("item five"); done[i] = 1; return GL_OK; });
    if (st != GL_ERR_INTERNAL || !strstr(gl_last_error(), "item five")) bad("lanes: std::runtime_error in a lane", 5, gl_last_error());
    printf("lanes: std::runtime_error became GL_ERR_INTERNAL\n");
    // the first failing status and ITS text come back unchanged, and the failing lane takes no further item (5 and 9 are lane 1's)
    reset();
    st = gl_run_lanes(4, 10, "abi_unwind", [&](size_t, size_t i) -> int { if (i == 1) return gl_fail(GL_ERR_ARG, "item one", "somewhere", 1); done[i] = 1; return GL_OK; });
    if (st != GL_ERR_ARG || strcmp(gl_last_error(), "item one (somewhere:1)") || done[5] || done[9]) bad("lanes: first error", 1, gl_last_error());
    // lanes stop taking items once a failure is recorded: on one lane the order is fixed, items 0..2 are done and 4..9 never start
    reset();
    st = gl_run_lanes(1, 10, "abi_unwind", [&](size_t, size_t i) -> int { if (i == 3) return gl_fail(GL_ERR_ARG, "item three", __FILE__, __LINE__); done[i] = 1; return GL_OK; });
    if (st != GL_ERR_ARG || count() != 3 || !done[0] || !done[1] || !done[2]) bad("lanes: stop after the first error", 3, gl_last_error());
    printf("lanes: the first error came back with its own text and stopped its lane\n");
    // std::thread's constructor allocates: every one of those allocations fails in turn
    sweep("lanes: thread start", reset, [&] { return gl_run_lanes(4, 10, "abi_unwind", [&](size_t, size_t i) -> int { done[i] = 1; return GL_OK; }); }, yes,
          [&] { return (uint64_t)count(); }, nothing);
    if (count() != 10) bad("lanes: thread start", -1, "a clean run left items out");
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    const auto ds = rd(dir + "/desc.bin"), cap = rd(dir + "/cap.bin"), dg = rd(dir + "/dig.bin"), pr = rd(dir + "/proof.bin"), vd = rd(dir + "/vd.bin");
    if (ds.size() != sizeof(gl_circuit_desc) || cap.empty() || dg.size() != 32 || pr.empty() || vd.empty()) { printf("bad inputs\n"); return 2; }
    const gl_circuit_desc* desc = (const gl_circuit_desc*)ds.data();
    const uint64_t* capw = (const uint64_t*)cap.data();
    const uint64_t* digw = (const uint64_t*)dg.data();
    const size_t m = 2;

    // ---- host circuit: build (both configurations, both hashers), columns, classes, witness ----
    gl_host_circuit* hc = nullptr;
    gl_circuit_desc d;
    for (uint32_t zk = 0; zk < 2; zk++)
        for (uint32_t hasher = 0; hasher < 2; hasher++) {
            char name[96];
            snprintf(name, sizeof name, "gl_matmul_circuit_build_h(m=2, zero_knowledge=%u, hasher=%u)", zk, hasher);
            sweep(name, [&] { hc = nullptr; }, [&] { return gl_matmul_circuit_build_h(m, zk, hasher, &hc); }, [&] { return hc == nullptr; },
                  [&] { return gl_host_circuit_desc(hc, &d) == GL_OK ? fnv(&d, sizeof d) : 0; }, [&] { gl_host_circuit_free(hc); hc = nullptr; });
        }
    auto build = [&] { hc = nullptr; if (gl_matmul_circuit_build_h(m, 0, 0, &hc) != GL_OK) abort(); };      // a fresh circuit: its sigma columns are computed on demand
    auto drop = [&] { gl_host_circuit_free(hc); hc = nullptr; };
    build();
    if (gl_host_circuit_desc(hc, &d) != GL_OK) return 2;
    const size_t n = size_t(1) << d.degree_bits;
    drop();
    std::vector<uint64_t> cs((d.num_constants + 80) * n), classes(80 * n), wires(135 * n), pis(3 * m * m);
    sweep("gl_host_circuit_constants_sigmas", build, [&] { return gl_host_circuit_constants_sigmas(hc, cs.data()); }, yes, [&] { return fnv(cs.data(), cs.size() * 8); }, drop, true);
    sweep("gl_host_circuit_wire_classes", build, [&] { return gl_host_circuit_wire_classes(hc, classes.data()); }, yes, [&] { return fnv(classes.data(), classes.size() * 8); }, drop, true);
    const uint64_t a[4] = {1, 2, 3, 4}, b[4] = {5, 6, 7, 8};
    sweep("gl_matmul_witness", build, [&] { return gl_matmul_witness(hc, a, b, 7, wires.data(), pis.data()); }, yes,
          [&] { return fnv(pis.data(), pis.size() * 8, fnv(wires.data(), wires.size() * 8)); }, drop, true);

    // ---- challenger ----
    for (uint32_t hasher = 0; hasher < 2; hasher++) {
        gl_challenger* ch = nullptr;
        uint64_t out[5], state[12], buf[8]; uint32_t len = 0;
        char name[96];
        snprintf(name, sizeof name, "gl_challenger_new_h(%u) + observe + get_challenges + state", hasher);
        sweep(name, [&] { ch = nullptr; },
              [&] {
                  if (!ch) ch = gl_challenger_new_h(hasher);
                  if (!ch) return GL_ERR_INTERNAL;
                  GL_TRY(gl_challenger_observe(ch, capw, 11));
                  GL_TRY(gl_challenger_observe_hashes(ch, 0, digw, 1));
                  GL_TRY(gl_challenger_get_challenges(ch, out, 5));
                  GL_TRY(gl_challenger_observe(ch, capw, 3));
                  return gl_challenger_state(ch, state, buf, &len);
              },
              [&] { return ch == nullptr; }, [&] { return fnv(out, sizeof out, fnv(state, sizeof state, fnv(buf, 8 * len))); }, [&] { gl_challenger_free(ch); ch = nullptr; }, true);
    }

    // ---- verifier and the circuit data as bytes ----
    sweep("gl_verify", nothing, [&] { return gl_verify(desc, capw, digw, pr.data(), pr.size()); }, yes, [] { return uint64_t(1); }, nothing);
    sweep("gl_host_circuit_verify", build, [&] { return gl_host_circuit_verify(hc, capw, digw, pr.data(), pr.size()); }, yes, [] { return uint64_t(1); }, drop, true);
    std::vector<uint8_t> bytes(1 << 20); size_t nb = 0, used = 0;
    sweep("gl_common_data_to_bytes", nothing, [&] { return gl_common_data_to_bytes(desc, bytes.data(), bytes.size(), &nb); }, yes, [&] { return fnv(bytes.data(), nb); }, nothing);
    const std::vector<uint8_t> common(bytes.begin(), bytes.begin() + nb);
    sweep("gl_common_data_from_bytes", nothing, [&] { return gl_common_data_from_bytes(common.data(), common.size(), &d, &used); }, yes,
          [&] { return fnv(&d, sizeof d, used); }, nothing);
    sweep("gl_verifier_only_to_bytes_h", nothing, [&] { return gl_verifier_only_to_bytes_h(0, desc->cap_height, capw, digw, bytes.data(), bytes.size(), &nb); }, yes,
          [&] { return fnv(bytes.data(), nb); }, nothing);
    const std::vector<uint8_t> only(bytes.begin(), bytes.begin() + nb);
    std::vector<uint64_t> cap_back(cap.size() / 8); uint64_t dig_back[4]; uint32_t cap_height = 0;
    sweep("gl_verifier_only_from_bytes_h", nothing,
          [&] { return gl_verifier_only_from_bytes_h(0, only.data(), only.size(), &cap_height, cap_back.data(), cap_back.size(), dig_back, &used); }, yes,
          [&] { return fnv(cap_back.data(), cap_back.size() * 8, fnv(dig_back, 32, cap_height)); }, nothing);
    sweep("gl_verify_bytes", nothing, [&] { return gl_verify_bytes(vd.data(), vd.size(), pr.data(), pr.size()); }, yes, [] { return uint64_t(1); }, nothing);
    {   // gl_verify_openings on a FriProof assembled here: one oracle holding the constant polynomial c (n = 8, rate_bits 1, cap_height 1),
        // opened at one point.  Its quotient is zero, so the codeword, the one reduction (arity 8) and the final polynomial are zero; every
        // leaf of the initial tree is [c], every node of a level the same hash.
        gl_fri_params fp = {};
        fp.degree_bits = 3; fp.rate_bits = 1; fp.cap_height = 1; fp.num_query_rounds = 2; fp.num_fri_rounds = 1; fp.fri_arity_bits[0] = 3;
        const uint32_t polys[2] = {0, 0};
        gl_fri_instance fi = {};
        fi.num_oracles = 1; fi.oracle_num_polys[0] = 1; fi.num_batches = 1; fi.points[0][0] = 5; fi.batch_len[0] = 1; fi.polys = polys;
        const uint64_t c = 0x1234567, leaf[1] = {c}, opening[2] = {c, 0}, zeros[16] = {0};
        uint64_t level[4][4], step_leaf[4];
        if (gl_hash_or_noop_host(0, leaf, 1, 1, level[0]) != GL_OK || gl_hash_or_noop_host(0, zeros, 1, 16, step_leaf) != GL_OK) abort();
        for (int l = 0; l < 3; l++) if (gl_two_to_one_host(0, level[l], level[l], 1, level[l + 1]) != GL_OK) abort();
        uint64_t caps[8];
        for (int i = 0; i < 8; i++) caps[i] = level[3][i % 4];
        std::vector<uint8_t> fproof;
        auto word = [&](uint64_t v) { for (int i = 0; i < 8; i++) fproof.push_back((uint8_t)(v >> (8 * i))); };
        for (int i = 0; i < 8; i++) word(step_leaf[i % 4]);                       // the commit cap: both leaves of the zero codeword's tree
        for (int q = 0; q < 2; q++) {
            word(c); fproof.push_back(3);
            for (int l = 0; l < 3; l++) for (int k = 0; k < 4; k++) word(level[l][k]);
            for (int i = 0; i < 16; i++) word(0);
            fproof.push_back(0);
        }
        word(0); word(0); word(0);                                                // the final polynomial (one coefficient) and the PoW witness
        gl_challenger* ch = nullptr;
        uint32_t code = 99;
        sweep("gl_verify_openings", [&] { ch = gl_challenger_new_h(0); if (!ch) abort(); code = 99; },
              [&] { return gl_verify_openings(&fp, &fi, caps, opening, ch, fproof.data(), fproof.size(), &code); }, yes, [&] { return uint64_t(code); },
              [&] { gl_challenger_free(ch); ch = nullptr; });
    }

    // ---- the context's entry points over the stub runtime (the stub's own allocations on the calling thread fail in turn too) ----
    gl_ctx* ctx = nullptr;
    sweep("context: gl_ctx_create + gl_ctx_destroy", [&] { ctx = nullptr; },
          [&] { GL_TRY(gl_ctx_create(0, nullptr, &ctx)); gl_ctx_destroy(ctx); ctx = nullptr; return GL_OK; }, [&] { return ctx == nullptr; },
          [] { return uint64_t(1); }, nothing, true);
    void* dev = nullptr;
    std::vector<uint64_t> src(4096), back(4096);
    for (size_t i = 0; i < src.size(); i++) src[i] = 0xC0FFEE00 + i;
    sweep("context: gl_dev_alloc + gl_copy_h2d + gl_copy_d2h + gl_ctx_synchronize", [&] { ctx = make_ctx(); dev = nullptr; },
          [&] {
              if (!dev) GL_TRY(gl_dev_alloc(ctx, src.size() * 8, &dev));
              GL_TRY(gl_copy_h2d(ctx, dev, src.data(), src.size() * 8));
              GL_TRY(gl_copy_d2h(ctx, back.data(), dev, back.size() * 8));
              return gl_ctx_synchronize(ctx);
          },
          yes, [&] { return fnv(back.data(), back.size() * 8); }, [&] { (void)gl_dev_free(ctx, dev); gl_ctx_destroy(ctx); }, true);
    char report[4096];
    sweep("context: gl_ctx_timing_report", [&] {
              ctx = make_ctx();
              if (gl_ctx_timing_enable(ctx, 1) != GL_OK) abort();
              for (int i = 0; i < 3; i++) { GlTimed outer(ctx, "outer"); GlTimed inner(ctx, i ? "inner" : "first"); }
          },
          [&] { return gl_ctx_timing_report(ctx, report, sizeof report); }, yes, [&] { return fnv(report, strlen(report)); },
          [&] { (void)gl_ctx_timing_reset(ctx); gl_ctx_destroy(ctx); }, true);
    // the stream-ordered pool is C++ behind the entry points: its exceptions are the caller's guard's, here gl_caught()
    void* block = nullptr;
    sweep("context: gl_ctx::pool_alloc", [&] { ctx = make_ctx(); block = nullptr; },
          [&] { try { return ctx->pool_alloc(size_t(3) << 16, &block); } catch (...) { return gl_caught(); } }, [&] { return block == nullptr; },
          [&] { return (uint64_t)ctx->pool_bytes; }, [&] { ctx->pool_release(block); gl_ctx_destroy(ctx); }, true);
    {   // pool_release is noexcept (destructors call it): without a node for its free list the block goes back to the runtime
        ctx = make_ctx();
        if (ctx->pool_alloc(size_t(3) << 16, &block) != GL_OK) abort();
        t_count = 0; t_fail_at = 0;
        ctx->pool_release(block);
        t_fail_at = -1;
        if (ctx->pool_bytes != 0 || !ctx->pool_free_blocks.empty() || !ctx->pool_block_size.empty()) bad("context: gl_ctx::pool_release", 0, "the block is still counted");
        printf("context: gl_ctx::pool_release: %ld allocations, the failing one gave the block back\n", t_count);
        gl_ctx_destroy(ctx);
    }

    lane_cases();
    printf("%d bad\n", g_bad);
    return g_bad ? 1 : 0;
}
