// Correctness of every function of the device branch of gl64_gfx950.cuh, one application per element, against the host's
// unsigned __int128 arithmetic: the value mod p, < p wherever the header promises a canonical result, and for glx_mad_k /
// glx_mac_c / glx_add_eps_if / glx_mk64 (a glx_u32x2 as a register pair) the exact 64-bit word.  No timing.  (GlxWideAcc2:
// tools/ubench/wide_acc.hip.)
//
// Inputs: the 164-value edge grid of tools/ubench/gl_prims.hip crossed with itself, the products of the S-boxes of 2^48, 2^24 and
// 2^14 (x x, x^2 x^2 and x^3 x^4 then subtract EPS without a carry: the cold block of glx_mul<false> / glx_mul3<false>), random
// words up to 2^17 elements; for the four products also WAVES built with the host model of the tail, since the cold block is
// chosen per wave: one borrow-only lane at lane 0 / 31 / 32 / 63 among lanes that add EPS and lanes without a fix-up (for
// glx_mul3 in slot A only, B only, C only), all lanes borrow-only, borrow-only inputs only in lanes a lane-dependent `if` has
// switched off and only in the lanes it has left on, and a last, partial wave.
// For each function the host counts the cases per class of its fix-up; an empty class that the function has is a failure (the
// run would be vacuous).  One line per function, `name: ok (cases, per-class counts)`; exit status = number of failing functions.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -I plonky2_demo_amd/csrc tools/ubench/glx_check.hip -o tools/ubench/bin/glx_check
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "gl64.cuh"
#include "gl64_gfx950.cuh"

typedef uint32_t u32;
typedef uint64_t u64;
typedef unsigned __int128 u128;
static const u64 P = 0xFFFFFFFF00000001ULL, EPS = 0xFFFFFFFFULL, M32 = 0xFFFFFFFFULL, SENTINEL = 0xDEADBEEFDEADBEEFULL;
static u64 h_mod(u128 x) { return (u64)(x % P); }
static u64 splitmix(u64& s) { u64 z = (s += 0x9E3779B97F4A7C15ULL); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(200); } } while (0)

// ------------------------------------------------------------------------------------------------------------- kernels
// `mask` (may be null): lanes whose byte is 0 skip the function and store the sentinel -- the function then runs under a partial
// EXEC mask.  Every store is inside i < n: the arrays are exactly n long.
template <typename F>
__global__ __launch_bounds__(256) void k_apply2(F f, const u64* a, const u64* b, const uint8_t* mask, u64* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) { o[i] = SENTINEL; return; }
    o[i] = f(a[i], b[i]);
}
// slot-major arrays of 3 n (4 n): thread i takes element i of every slot
template <bool CANON>
__global__ __launch_bounds__(256) void k_mul3(const u64* a, const u64* b, const uint8_t* mask, u64* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) { o[i] = SENTINEL; o[n + i] = SENTINEL; o[2 * n + i] = SENTINEL; return; }
    gl_t rA, rB, rC;
    glx_mul3<CANON>(a[i], b[i], a[n + i], b[n + i], a[2 * n + i], b[2 * n + i], rA, rB, rC);
    o[i] = rA; o[n + i] = rB; o[2 * n + i] = rC;
}
__global__ __launch_bounds__(256) void k_sub4(const u64* a, const u64* b, u64* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const gl_t x[4] = {a[i], a[n + i], a[2 * n + i], a[3 * n + i]}, y[4] = {b[i], b[n + i], b[2 * n + i], b[3 * n + i]};
    gl_t r[4];
    glx_sub_cc4(x, y, r);
    for (int k = 0; k < 4; k++) o[k * n + i] = r[k];
}
__global__ __launch_bounds__(256) void k_acc3(const u64* al, const u64* ah, u64* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gl_t rA, rB, rC;
    glx_acc_reduce3(al[i], ah[i], al[n + i], ah[n + i], al[2 * n + i], ah[2 * n + i], rA, rB, rC);
    o[i] = rA; o[n + i] = rB; o[2 * n + i] = rC;
}
// slots 0..2 of a / b: the lo accumulators before their last term / that term as x | c << 32; slots 3..5: the hi accumulators
__global__ __launch_bounds__(256) void k_acc3w(const u64* acc, const u64* term, u64* o, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    gl_t al[3], ah[3], r[3];
    uint64_t wl[3], wh[3];
    for (int k = 0; k < 3; k++) {
        const u64 tl = term[k * n + i], th = term[(3 + k) * n + i];
        al[k] = glx_mac_co(acc[k * n + i], (u32)tl, __builtin_amdgcn_readfirstlane((u32)(tl >> 32)), wl[k]);
        ah[k] = glx_mac_co(acc[(3 + k) * n + i], (u32)th, __builtin_amdgcn_readfirstlane((u32)(th >> 32)), wh[k]);
    }
    glx_acc_reduce3w(al[0], ah[0], wl[0], wh[0], al[1], ah[1], wl[1], wh[1], al[2], ah[2], wl[2], wh[2], r[0], r[1], r[2]);
    for (int k = 0; k < 3; k++) { o[k * n + i] = r[k]; o[(3 + k) * n + i] = 0; }
}

template <bool CANON> struct F_mul { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_mul<CANON>(a, b); } };
struct F_add_cc { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_add_cc(a, b); } };
struct F_add_1c { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_add_1c(a, b); } };
struct F_sub_cc { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_sub_cc(a, b); } };
struct F_canon { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t) const { return glx_canon(a); } };
struct F_add_eps_if { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_add_eps_if(a, (u32)b & 1u); } };
struct F_reduce96 { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_reduce96(a, (u32)b); } };
struct F_acc_reduce { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_acc_reduce(a, b); } };
// the register pair: glx_mk64 against the two lanes of a glx_u32x2 read back
// (glx_mk64, glx_u32x2 and glx_fix_canon exist in the device pass only)
struct F_mk64 {
    __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const {
#if defined(__HIP_DEVICE_COMPILE__)
        const gl_t r = glx_mk64((u32)a, (u32)b);
        const glx_u32x2 v = __builtin_bit_cast(glx_u32x2, r);
        return (v.x == (u32)a && v.y == (u32)b) ? r : ~r;
#else
        return a + b;
#endif
    }
};
// the carry mask of glx_fix_canon is a wave mask in scalar registers: the ballot of bit 0 of b
struct F_fix_canon {
    __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return glx_fix_canon(a, __ballot((int)(b & 1)));
#else
        return a + b;
#endif
    }
};
template <u32 C> struct F_mad_k { u64 k; __device__ __forceinline__ gl_t operator()(gl_t a, gl_t) const { return glx_mad_k((u32)a, C, k); } };
template <u32 C> struct F_mac_c { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t b) const { return glx_mac_c(a, (u32)b, C); } };
template <int E> struct F_shl { __device__ __forceinline__ gl_t operator()(gl_t a, gl_t) const { return glx_shl_c<E>(a); } };

// ---------------------------------------------------------------------------------- the host model of a product's tail
// (tests/test_product_rare_fixup.py product_parts / masks): y = lo + w2 EPS - hh (mod 2^64), carry c of the sum, borrow bw
struct Parts { u64 y; int c, bw; };
static Parts product_parts(u64 a, u64 b) {
    const u64 a0 = a & M32, a1 = a >> 32, b0 = b & M32, b1 = b >> 32;
    const u64 p00 = a0 * b0, p11 = a1 * b1;
    const u128 mid128 = (u128)(a0 * b1) + (u128)(a1 * b0);
    const u64 cm = (u64)(mid128 >> 64), mid = (u64)mid128;
    u64 s = (p00 >> 32) + (mid & M32);
    const u64 w1 = s & M32;
    s = (p11 & M32) + (mid >> 32) + (s >> 32);
    const u64 w2 = s & M32, w3 = (p11 >> 32) + (s >> 32);
    const u128 z128 = (u128)((w1 << 32) | (p00 & M32)) + (u128)w2 * EPS;
    const u64 z = (u64)z128, hh = w3 + cm;
    return {z - hh, (int)(z128 >> 64), z < hh ? 1 : 0};
}
enum { SUB = 0, ADD = 1, NONE = 2, BOTH = 3, GE_P = 4 };       // subtract EPS (the cold block) | add EPS | neither | carry and borrow | CANON: y >= p
static int product_class(u64 a, u64 b, bool canon) {
    const Parts t = product_parts(a, b);
    if (t.bw && !t.c) return SUB;
    if (t.c && !t.bw) return ADD;
    if (t.c && t.bw) return BOTH;              // (y = z - hh has wrapped: CANON then finds y >= p as well)
    return (canon && t.y >= P) ? GE_P : NONE;
}

// --------------------------------------------------------------------------------------------------------- reporting
static int g_failed = 0;
struct Tally {
    std::string name;
    std::vector<const char*> classes;
    std::vector<size_t> count;
    unsigned required;                     // bit k: class k must not stay empty
    size_t cases = 0, bad = 0;
    Tally(std::string n, std::vector<const char*> c, unsigned req) : name(std::move(n)), classes(std::move(c)), count(classes.size(), 0), required(req) {}
    void mismatch(u64 a, u64 b, u64 got, u64 want, const char* what) {
        if (bad++ < 3) printf("  %s MISMATCH %s a=%016llx b=%016llx got=%016llx want=%016llx\n", name.c_str(), what, (unsigned long long)a, (unsigned long long)b,
                              (unsigned long long)got, (unsigned long long)want);
    }
    void note(const char* text) { if (bad++ < 3) printf("  %s: %s\n", name.c_str(), text); }
    bool finish() {
        bool ok = bad == 0 && cases > 0;
        std::string s;
        for (size_t k = 0; k < classes.size(); k++) {
            s += (k ? ", " : ""); s += classes[k]; s += " " + std::to_string(count[k]);
            if (((required >> k) & 1) && !count[k]) { ok = false; printf("  %s: no case of class '%s': the run would be vacuous\n", name.c_str(), classes[k]); }
        }
        printf("%s: %s (%zu cases%s%s)\n", name.c_str(), ok ? "ok" : "FAIL", cases, s.empty() ? "" : "; ", s.c_str());
        if (!ok) g_failed++;
        return ok;
    }
};

struct Dev {
    u64 *a = nullptr, *b = nullptr, *o = nullptr; uint8_t* m = nullptr; size_t cap = 0;
    void reserve(size_t n) {
        if (n <= cap) return;
        if (a) { HIP_OK(hipFree(a)); HIP_OK(hipFree(b)); HIP_OK(hipFree(o)); HIP_OK(hipFree(m)); }
        HIP_OK(hipMalloc((void**)&a, n * 8)); HIP_OK(hipMalloc((void**)&b, n * 8)); HIP_OK(hipMalloc((void**)&o, n * 8)); HIP_OK(hipMalloc((void**)&m, n));
        cap = n;
    }
};
static Dev g_dev;
static unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// upload (a, b[, mask]), run, download into out
template <typename F>
static void run2(F f, const std::vector<u64>& a, const std::vector<u64>& b, const std::vector<uint8_t>* mask, std::vector<u64>& out) {
    const size_t n = a.size();
    g_dev.reserve(n);
    HIP_OK(hipMemcpy(g_dev.a, a.data(), n * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(g_dev.b, b.data(), n * 8, hipMemcpyHostToDevice));
    if (mask) HIP_OK(hipMemcpy(g_dev.m, mask->data(), n, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(g_dev.o, 0x5A, n * 8));
    hipLaunchKernelGGL(k_apply2<F>, dim3(blocks_for(n)), dim3(256), 0, 0, f, g_dev.a, g_dev.b, mask ? g_dev.m : nullptr, g_dev.o, n);
    HIP_OK(hipGetLastError());
    out.resize(n);
    HIP_OK(hipMemcpy(out.data(), g_dev.o, n * 8, hipMemcpyDeviceToHost));
}
// slot-major arrays of `slots` x n through one of the multi-slot kernels
template <typename Launch>
static void run_slots(Launch launch, int slots, size_t n, const std::vector<u64>& a, const std::vector<u64>& b, const std::vector<uint8_t>* mask, std::vector<u64>& out) {
    g_dev.reserve((size_t)slots * n);
    HIP_OK(hipMemcpy(g_dev.a, a.data(), slots * n * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(g_dev.b, b.data(), slots * n * 8, hipMemcpyHostToDevice));
    if (mask) HIP_OK(hipMemcpy(g_dev.m, mask->data(), n, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(g_dev.o, 0x5A, slots * n * 8));
    launch(g_dev.a, g_dev.b, mask ? g_dev.m : nullptr, g_dev.o, n);
    HIP_OK(hipGetLastError());
    out.resize((size_t)slots * n);
    HIP_OK(hipMemcpy(out.data(), g_dev.o, slots * n * 8, hipMemcpyDeviceToHost));
}

// ------------------------------------------------------------------------------------------- waves for the products
typedef std::pair<u64, u64> Pair;
struct Pools { std::vector<Pair> sub, add, none; size_t is = 0, ia = 0, in_ = 0;
    Pair next_sub() { return sub[is++ % sub.size()]; }
    Pair next_other(size_t lane) { return (lane & 1) ? add[ia++ % add.size()] : none[in_++ % none.size()]; } };
// One launch of `slots` products per lane.  The borrow-only pairs go to slot `hot` (all = true: to every slot, in the all-borrow
// wave).  want_sub[w][s]: how many ACTIVE lanes of wave w are borrow-only in slot s, as built; main() recounts it with the model.
struct Shaped { std::vector<u64> a, b; std::vector<uint8_t> mask; size_t n = 0; std::vector<std::vector<int>> want_sub; std::vector<const char*> shape; };
static Shaped build_shapes(Pools& pl, int slots, int hot) {
    struct Wave { const char* shape; int lanes; int (*sub_lane)(int); int (*active)(int); bool every_slot; };
    static const Wave waves[] = {
        {"one at lane 0", 64, [](int l) { return l == 0 ? 1 : 0; }, [](int) { return 1; }, false},
        {"one at lane 31", 64, [](int l) { return l == 31 ? 1 : 0; }, [](int) { return 1; }, false},
        {"one at lane 32", 64, [](int l) { return l == 32 ? 1 : 0; }, [](int) { return 1; }, false},
        {"one at lane 63", 64, [](int l) { return l == 63 ? 1 : 0; }, [](int) { return 1; }, false},
        {"all lanes", 64, [](int) { return 1; }, [](int) { return 1; }, false},
        {"all lanes, all slots", 64, [](int) { return 1; }, [](int) { return 1; }, true},
        {"only in switched-off lanes", 64, [](int l) { return l % 3 == 0 ? 1 : 0; }, [](int l) { return l % 3 == 0 ? 0 : 1; }, false},
        {"only in the lanes left on", 64, [](int l) { return l % 3 == 0 ? 1 : 0; }, [](int l) { return l % 3 == 0 ? 1 : 0; }, false},
        {"none (fast tail only)", 64, [](int) { return 0; }, [](int) { return 1; }, false},
        {"partial last wave", 37, [](int l) { return l == 5 ? 1 : 0; }, [](int) { return 1; }, false},
    };
    Shaped s;
    for (const Wave& w : waves) s.n += w.lanes;
    s.a.assign(slots * s.n, 0); s.b.assign(slots * s.n, 0); s.mask.assign(s.n, 1);
    size_t base = 0;
    for (const Wave& w : waves) {
        std::vector<int> want(slots, 0);
        for (int l = 0; l < w.lanes; l++) {
            s.mask[base + l] = (uint8_t)w.active(l);
            for (int sl = 0; sl < slots; sl++) {
                const bool sub = w.sub_lane(l) && (sl == hot || w.every_slot);
                const Pair p = sub ? pl.next_sub() : pl.next_other(l + sl);
                s.a[sl * s.n + base + l] = p.first; s.b[sl * s.n + base + l] = p.second;
                if (sub && w.active(l)) want[sl]++;
            }
        }
        s.want_sub.push_back(want); s.shape.push_back(w.shape);
        base += w.lanes;
    }
    return s;
}
// the shapes hold what they claim, by the model: per wave and slot the active borrow-only lanes; every full-mask wave with fewer
// than 64 of them also has lanes that add EPS and lanes without a fix-up
static bool shapes_hold(const Shaped& s, int slots, bool canon) {
    size_t base = 0;
    for (size_t w = 0; w < s.want_sub.size(); w++) {
        const size_t lanes = (w + 1 == s.want_sub.size()) ? s.n - base : 64;
        for (int sl = 0; sl < slots; sl++) {
            int sub = 0, add = 0, none = 0;
            for (size_t l = 0; l < lanes; l++) {
                if (!s.mask[base + l]) continue;
                const int c = product_class(s.a[sl * s.n + base + l], s.b[sl * s.n + base + l], canon);
                sub += c == SUB; add += c == ADD; none += c == NONE;
            }
            if (sub != s.want_sub[w][sl]) { printf("  shape '%s' slot %d: %d borrow-only lanes, built for %d\n", s.shape[w], sl, sub, s.want_sub[w][sl]); return false; }
            if (sub < (int)lanes / 3 && (!add || !none)) { printf("  shape '%s' slot %d: no mix of fix-ups\n", s.shape[w], sl); return false; }
        }
        base += lanes;
    }
    return true;
}

template <bool CANON>
static void check_products(const std::vector<u64>& ha, const std::vector<u64>& hb, Pools& pools) {
    const std::vector<const char*> cls = {"subtract", "add", "none", "carry and borrow", "y >= p"};
    const unsigned req = CANON ? 0x1F : 0x0F;
    std::vector<u64> out;
    auto judge = [&](Tally& t, u64 a, u64 b, u64 got, bool active) {
        t.cases++;
        if (!active) { if (got != SENTINEL) t.mismatch(a, b, got, SENTINEL, "(switched-off lane)"); return; }
        t.count[product_class(a, b, CANON)]++;
        const u64 want = h_mod((u128)a * b);
        if (got % P != want || (CANON && got >= P)) t.mismatch(a, b, got, want, "");
    };
    {   // the single product
        Tally t(CANON ? "glx_mul<true>" : "glx_mul<false>", cls, req);
        run2(F_mul<CANON>(), ha, hb, nullptr, out);
        for (size_t i = 0; i < ha.size(); i++) judge(t, ha[i], hb[i], out[i], true);
        Shaped s = build_shapes(pools, 1, 0);
        if (!shapes_hold(s, 1, CANON)) t.note("the crafted waves do not hold their shapes");
        run2(F_mul<CANON>(), s.a, s.b, &s.mask, out);
        for (size_t i = 0; i < s.n; i++) judge(t, s.a[i], s.b[i], out[i], s.mask[i]);
        t.finish();
    }
    {   // three at a time: every pair of the flat arrays in every slot (slot k is the arrays rotated by 11 k), then the waves with the
        // borrow-only lanes in slot A only, B only, C only
        Tally t(CANON ? "glx_mul3<true>" : "glx_mul3<false>", cls, req);
        auto launch = [](const u64* a, const u64* b, const uint8_t* m, u64* o, size_t n) { hipLaunchKernelGGL(k_mul3<CANON>, dim3(blocks_for(n)), dim3(256), 0, 0, a, b, m, o, n); };
        const size_t n = ha.size();
        std::vector<u64> a3(3 * n), b3(3 * n);
        for (int k = 0; k < 3; k++) for (size_t i = 0; i < n; i++) { a3[k * n + i] = ha[(i + 11 * k) % n]; b3[k * n + i] = hb[(i + 11 * k) % n]; }
        run_slots(launch, 3, n, a3, b3, nullptr, out);
        for (size_t i = 0; i < 3 * n; i++) judge(t, a3[i], b3[i], out[i], true);
        for (int hot = 0; hot < 3; hot++) {
            Shaped s = build_shapes(pools, 3, hot);
            if (!shapes_hold(s, 3, CANON)) t.note("the crafted waves do not hold their shapes");
            run_slots(launch, 3, s.n, s.a, s.b, &s.mask, out);
            for (size_t i = 0; i < 3 * s.n; i++) judge(t, s.a[i], s.b[i], out[i], s.mask[i % s.n]);
        }
        t.finish();
    }
}

// a two-operand function on flat arrays: ref gives the wanted value (exact: the wanted word), cls the class of the case
template <typename F, typename Ref, typename Cls>
static void check2(const char* name, F f, const std::vector<u64>& a, const std::vector<u64>& b, Ref ref, Cls cls, std::vector<const char*> classes, unsigned req,
                   bool canon_out, bool exact, Tally* into = nullptr) {
    Tally own(name, std::move(classes), req);
    Tally& t = into ? *into : own;
    std::vector<u64> out;
    run2(f, a, b, nullptr, out);
    for (size_t i = 0; i < a.size(); i++) {
        t.cases++;
        t.count[cls(a[i], b[i])]++;
        const u64 want = ref(a[i], b[i]);
        const bool ok = exact ? out[i] == want : (out[i] % P == want % P && (!canon_out || out[i] < P));
        if (!ok) t.mismatch(a[i], b[i], out[i], want, "");
    }
    if (!into) own.finish();
}

static constexpr u32 MDS_CONSTANTS[] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20, 25};      // circ[0..11] and M[0][0] = 17 + 8
template <u32 C>
static void check_mad_mac(const std::vector<u64>& a, const std::vector<u64>& b, Tally& mad, Tally& mac) {
    // glx_mad_k: x * c + k for wave-uniform k (a kernel argument); glx_mac_c: acc + x * c.  Exact words.
    for (u64 k : {0ULL, 1ULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFF00000000ULL, 0x00000000FFFFFFFFULL, 0xB585F766F2144405ULL}) {
        F_mad_k<C> f; f.k = k;
        check2("glx_mad_k", f, a, b, [k](u64 x, u64) { return (u64)(x & M32) * C + k; }, [k](u64 x, u64) { return ((u128)((x & M32) * C) + k) >> 64 ? 0 : 1; }, {}, 0, false, true, &mad);
    }
    check2("glx_mac_c", F_mac_c<C>(), a, b, [](u64 acc, u64 x) { return acc + (x & M32) * C; }, [](u64 acc, u64 x) { return ((u128)acc + (x & M32) * C) >> 64 ? 0 : 1; }, {}, 0, false, true, &mac);
}
template <size_t... I>
static void check_all_mad_mac(const std::vector<u64>& a, const std::vector<u64>& b, Tally& mad, Tally& mac, std::index_sequence<I...>) {
    (check_mad_mac<MDS_CONSTANTS[I]>(a, b, mad, mac), ...);
}

// glx_shl_c<E>: canonical in, canonical out.  Classes by the branch of E: E <= 32 one fix-up (carry or >= p); 32 < E < 64 the
// product's two-sided fix-up; E >= 64 a canonical difference (borrow or not).
template <int E>
static void check_shl(const std::vector<u64>& x) {
    u64 pw = 1;
    for (int i = 0; i < E; i++) pw = h_mod((u128)pw * 2);
    auto ref = [pw](u64 v, u64) { return h_mod((u128)v * pw); };
    const std::string name = "glx_shl_c<" + std::to_string(E) + ">";
    if constexpr (E <= 32) {
        auto cls = [](u64 v, u64) {                  // (h:m:l) = x << E: (m:l) + h EPS
            const u64 h = E == 32 ? v >> 32 : v >> (64 - E);
            const u128 s = (u128)(u64)(v << E) + (u128)h * EPS;
            return (s >> 64 || (u64)s >= P) ? 0 : 1;
        };
        check2(name.c_str(), F_shl<E>(), x, x, ref, cls, {"fix-up", "none"}, 0x3, true, false);
    } else if constexpr (E < 64) {
        auto cls = [](u64 v, u64) {
            const u64 a = v << E, u = v >> (64 - E);
            const u128 z128 = (u128)a + (u128)(u & M32) * EPS;
            const u64 z = (u64)z128, h = u >> 32;
            const int c = (int)(z128 >> 64), bw = z < h;
            return (bw && !c) ? 0 : (c && !bw) ? 1 : (z - h >= P) ? 2 : 3;
        };
        check2(name.c_str(), F_shl<E>(), x, x, ref, cls, {"subtract", "add", "y >= p", "none"}, 0xB, true, false);
    } else {
        auto cls = [](u64 v, u64) { constexpr int R = E - 64; return (u64)((u32)v << R) * EPS < (v >> (32 - R)) ? 0 : 1; };
        check2(name.c_str(), F_shl<E>(), x, x, ref, cls, {"borrow", "none"}, 0x3, true, false);
    }
}
template <int... E>
static void check_all_shl(const std::vector<u64>& x, std::integer_sequence<int, E...>) { (check_shl<E + 1>(x), ...); }

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    // the edge grid of gl_prims.hip (gl_prims_grid() of tests/test_product_rare_fixup.py)
    const u64 edge[] = {0, 1, 2, P - 1, P, P + 1, 0xFFFFFFFFULL, 0x100000000ULL, 0xFFFFFFFFFFFFFFFFULL, 0xFFFFFFFF00000000ULL, 0xFFFFFFFEFFFFFFFFULL,
                        0x8000000000000000ULL, 0x7FFFFFFFFFFFFFFFULL, 0xFFFFFFFF, 0xFFFFFFFE00000001ULL, 0x00000001FFFFFFFFULL};
    std::vector<u64> grid(edge, edge + sizeof(edge) / sizeof(edge[0]));
    for (int k = 0; k < 64; k++) { grid.push_back(1ULL << k); grid.push_back(P - (1ULL << k)); }
    for (int E : {36, 48, 60}) for (u64 h : {1ULL, 3ULL, 7ULL, (1ULL << (E - 33)) + 1, (1ULL << (E - 32)) - 1}) grid.push_back(h << (96 - E));
    for (int E : {12, 24, 36, 48, 60}) grid.push_back((0xFEDCBA9876543210ULL >> (64 - E)) << (64 - E));
    if (grid.size() != 164) { printf("the grid has %zu values, not 164\n", grid.size()); return 201; }
    std::vector<u64> ha, hb;
    for (u64 x : grid) for (u64 y : grid) { ha.push_back(x); hb.push_back(y); }
    // the four products of the S-box of 2^48 (x x), 2^24 (x^2 x^2) and 2^14 (x^3 x^4): each reaches the cold block once
    int sbox_cold = 0;
    for (u64 x : {1ULL << 48, 1ULL << 24, 1ULL << 14}) {
        const u64 x2 = h_mod((u128)x * x), x4 = h_mod((u128)x2 * x2), x3 = h_mod((u128)x * x2);
        for (Pair p : {Pair(x, x), Pair(x2, x2), Pair(x, x2), Pair(x3, x4)}) { ha.push_back(p.first); hb.push_back(p.second); sbox_cold += product_class(p.first, p.second, false) == SUB; }
    }
    if (sbox_cold < 3) { printf("the S-box inputs 2^48, 2^24, 2^14 reach the cold block %d times, not 3\n", sbox_cold); return 202; }
    u64 seed = 12345;
    while (ha.size() < (1u << 17)) { ha.push_back(splitmix(seed)); hb.push_back(splitmix(seed)); }
    const size_t n = ha.size();
    std::vector<u64> hac(ha), hbc(hb);
    for (auto& v : hac) v %= P;
    for (auto& v : hbc) v %= P;

    // ---- the products
    Pools pools;
    for (u64 x : grid) for (u64 y : grid) {
        const int c = product_class(x, y, false), cc = product_class(x, y, true);
        if (c == SUB && cc == SUB) pools.sub.push_back({x, y});
        else if (c == ADD && cc == ADD) pools.add.push_back({x, y});
        else if (c == NONE && cc == NONE) pools.none.push_back({x, y});
    }
    if (pools.sub.size() < 64 || pools.add.size() < 64 || pools.none.size() < 64) { printf("the grid gives too few pairs per class\n"); return 203; }
    check_products<false>(ha, hb, pools);
    check_products<true>(ha, hb, pools);

    // ---- canonical sums and differences
    auto radd = [](u64 a, u64 b) { return h_mod((u128)a + b); };
    auto rsub = [](u64 a, u64 b) { return h_mod((u128)a + P - b); };
    check2("glx_add_cc", F_add_cc(), hac, hbc, radd, [](u64 a, u64 b) { const u128 s = (u128)a + b; return s >> 64 ? 0 : (u64)s >= P ? 1 : 2; }, {"carry", ">= p", "none"}, 0x7, true, false);
    // glx_add_1c: any word plus a canonical one; the exact word (the wrapped sum + EPS where it wrapped), a representative of the sum
    check2("glx_add_1c", F_add_1c(), ha, hbc, [](u64 a, u64 b) { const u128 s = (u128)a + b; return (u64)s + (s >> 64 ? EPS : 0); },
           [](u64 a, u64 b) { return ((u128)a + b) >> 64 ? 0 : 1; }, {"carry", "none"}, 0x3, false, true);
    check2("glx_sub_cc", F_sub_cc(), hac, hbc, rsub, [](u64 a, u64 b) { return a < b ? 0 : 1; }, {"borrow", "none"}, 0x3, true, false);
    {
        Tally t("glx_sub_cc4", {"borrow", "none"}, 0x3);
        std::vector<u64> a4(4 * n), b4(4 * n), out;
        for (int k = 0; k < 4; k++) for (size_t i = 0; i < n; i++) { a4[k * n + i] = hac[(i + 7 * k) % n]; b4[k * n + i] = hbc[(i + 13 * k) % n]; }
        run_slots([](const u64* a, const u64* b, const uint8_t*, u64* o, size_t m) { hipLaunchKernelGGL(k_sub4, dim3(blocks_for(m)), dim3(256), 0, 0, a, b, o, m); }, 4, n, a4, b4, nullptr, out);
        for (size_t i = 0; i < 4 * n; i++) {
            t.cases++; t.count[a4[i] < b4[i] ? 0 : 1]++;
            if (out[i] != rsub(a4[i], b4[i])) t.mismatch(a4[i], b4[i], out[i], rsub(a4[i], b4[i]), i < n ? "slot 0" : i < 2 * n ? "slot 1" : i < 3 * n ? "slot 2" : "slot 3");
        }
        t.finish();
    }
    check2("glx_canon", F_canon(), ha, hb, [](u64 a, u64) { return a >= P ? a - P : a; }, [](u64 a, u64) { return a >= P ? 0 : 1; }, {"subtract p", "none"}, 0x3, true, true);
    check2("glx_add_eps_if", F_add_eps_if(), ha, hb, [](u64 a, u64 b) { return a + (b & 1) * EPS; }, [](u64 a, u64 b) { return (b & 1) ? ((((u128)a + EPS) >> 64) ? 0 : 1) : 2; },
           {"add, wraps", "add", "none"}, 0x7, false, true);
    check2("glx_mk64", F_mk64(), ha, hb, [](u64 a, u64 b) { return (b << 32) | (a & M32); }, [](u64, u64) { return 0; }, {"pairs"}, 0x1, false, true);
    {   // glx_fix_canon(z, carry): the value z + carry 2^64 is below 2 p; a set carry comes with z < 2^63 here
        std::vector<u64> z(ha), f(hb);
        for (size_t i = 0; i < n; i++) if (z[i] >> 63) f[i] &= ~1ULL;
        check2("glx_fix_canon", F_fix_canon(), z, f, [](u64 a, u64 b) { return h_mod((u128)a + ((u128)(b & 1) << 64)); }, [](u64 a, u64 b) { return (b & 1) ? 0 : a >= P ? 1 : 2; },
               {"carry", ">= p", "none"}, 0x7, true, false);
    }

    // ---- the accumulator folds: lo + top 2^64, and al + ah 2^32 with al, ah < 2^63
    check2("glx_reduce96", F_reduce96(), ha, hb, [](u64 lo, u64 top) { return h_mod((u128)lo + (u128)(top & M32) * EPS); },
           [](u64 lo, u64 top) { return ((u128)lo + (u128)(top & M32) * EPS) >> 64 ? 0 : 1; }, {"carry", "none"}, 0x3, false, false);
    std::vector<u64> al(ha), ah(hb);
    for (auto& v : al) v >>= 1;
    for (auto& v : ah) v >>= 1;
    auto racc = [](u64 l, u64 h) { return h_mod((u128)l + ((u128)h << 32)); };
    auto cacc = [](u64 l, u64 h) { const u128 s = (u128)l + ((u128)h << 32); return ((u128)(u64)s + (u128)(u64)(s >> 64) * EPS) >> 64 ? 0 : 1; };
    check2("glx_acc_reduce", F_acc_reduce(), al, ah, racc, cacc, {"carry", "none"}, 0x3, false, false);
    {
        Tally t("glx_acc_reduce3", {"carry", "none"}, 0x3);
        std::vector<u64> l3(3 * n), h3(3 * n), out;
        for (int k = 0; k < 3; k++) for (size_t i = 0; i < n; i++) { l3[k * n + i] = al[(i + 5 * k) % n]; h3[k * n + i] = ah[(i + 17 * k) % n]; }
        run_slots([](const u64* a, const u64* b, const uint8_t*, u64* o, size_t m) { hipLaunchKernelGGL(k_acc3, dim3(blocks_for(m)), dim3(256), 0, 0, a, b, o, m); }, 3, n, l3, h3, nullptr, out);
        for (size_t i = 0; i < 3 * n; i++) {
            t.cases++; t.count[cacc(l3[i], h3[i])]++;
            if (out[i] % P != racc(l3[i], h3[i])) t.mismatch(l3[i], h3[i], out[i], racc(l3[i], h3[i]), i < n ? "slot 0" : i < 2 * n ? "slot 1" : "slot 2");
        }
        t.finish();
    }

    {   // glx_mac_co + glx_acc_reduce3w: any 64-bit accumulator plus one 32 x 32 product as the last term, the wrap handed over as a mask.
        // The coefficient is wave-uniform (a scalar operand), so a wave of 64 elements shares one.
        Tally t("glx_acc_reduce3w", {"lo wraps", "hi wraps", "top carries", "lo and hi wrap", "none"}, 0x1F);
        const size_t m = ((std::min<size_t>(n, 164 * 164 + 12 + 16384) + 63) / 64 + 2) * 64;
        std::vector<u64> acc(6 * m), term(6 * m), out;
        const u32 coef[] = {0, 1, 0x1FFFFFFFu, 0xFFFFFFFFu, 0x16BD2D97u /* M^4[0][0] */};
        u64 seed = 99;
        for (int k = 0; k < 6; k++)
            for (size_t i = 0; i < m; i++) {
                const size_t wave = i / 64;
                u32 c = wave % 7 < 5 ? coef[(wave + k) % 5] : (u32)(splitmix(seed) >> 35);
                u64 a = k < 3 ? ha[(i + 5 * k) % n] : hb[(i + 17 * k) % n];
                u32 x = (u32)splitmix(seed);
                if (i % 5 == 0) x = 0xFFFFFFFFu;
                if (wave == m / 64 - 1) {          // the carry out of the top word: ah = 2^64 - 1 unwrapped, al.hi + ah.lo >= 2^32
                    x = 0; a = k < 3 ? ((u64)(1 + i % 3) << 32) + i : ~0ULL - (i % 2);
                }
                if (wave == m / 64 - 2) {          // and together with a wrapped lo accumulator
                    if (k < 3) { a = ~0ULL - i; x = 0xFFFFFFFFu; c = 0xFFFFFFFFu; } else { a = ~0ULL; x = 0; }
                }
                acc[k * m + i] = a; term[k * m + i] = (u64)x | ((u64)c << 32);
            }
        // one coefficient per wave and slot: copy lane 0's
        for (int k = 0; k < 6; k++) for (size_t i = 0; i < m; i++) term[k * m + i] = (term[k * m + i] & M32) | (term[k * m + (i & ~(size_t)63)] & ~M32);
        run_slots([](const u64* a, const u64* b, const uint8_t*, u64* o, size_t mm) { hipLaunchKernelGGL(k_acc3w, dim3(blocks_for(mm)), dim3(256), 0, 0, a, b, o, mm); }, 6, m, acc, term, nullptr, out);
        for (int k = 0; k < 3; k++)
            for (size_t i = 0; i < m; i++) {
                const u128 l = (u128)acc[k * m + i] + (u128)(term[k * m + i] & M32) * (term[k * m + i] >> 32);
                const u128 h = (u128)acc[(3 + k) * m + i] + (u128)(term[(3 + k) * m + i] & M32) * (term[(3 + k) * m + i] >> 32);
                const u64 want = h_mod(l + (h << 32));            // l, h < 2^65
                const bool wl = l >> 64, wh = h >> 64;
                const bool top = !wh && (u32)((u64)h >> 32) == 0xFFFFFFFFu && (((u64)l >> 32) + ((u64)h & M32)) >> 32;
                t.cases++;
                if (wl) t.count[0]++;
                if (wh) t.count[1]++;
                if (top) t.count[2]++;
                if (wl && wh) t.count[3]++;
                if (!wl && !wh && !top) t.count[4]++;
                if (out[k * m + i] % P != want) t.mismatch(acc[k * m + i], acc[(3 + k) * m + i], out[k * m + i], want, wl ? (wh ? "lo, hi" : "lo") : wh ? "hi" : top ? "top" : "none");
            }
        t.finish();
    }

    // ---- multiply-adds by the constants the Poseidon code passes (exact words), on the grid pairs and 2^13 random ones
    {
        std::vector<u64> sa(ha.begin(), ha.begin() + 164 * 164 + 12 + 8192), sb(hb.begin(), hb.begin() + 164 * 164 + 12 + 8192);
        Tally mad("glx_mad_k", {"wraps", "none"}, 0x3), mac("glx_mac_c", {"wraps", "none"}, 0x3);
        check_all_mad_mac(sa, sb, mad, mac, std::make_index_sequence<sizeof(MDS_CONSTANTS) / sizeof(MDS_CONSTANTS[0])>());
        mad.finish(); mac.finish();
    }

    // ---- every shift twiddle: the canonical grid, for 32 < E < 64 the forms h 2^(96 - E) (a zero low and middle word: borrow
    // without carry) with h = 1 and h = 2^(E - 32) - 1, for E <= 32 the least x with x 2^E >= j p (j = 1, 2, 3: (m:l) + h EPS lands on
    // p, p + 1, ...: the fix-up without a carry) and its predecessor, and 2^14 random canonical words
    {
        std::vector<u64> x;
        for (u64 v : grid) x.push_back(v % P);
        for (int E = 1; E <= 32; E++)
            for (u64 j = 1; j <= 3 && j < (1ULL << E); j++) { const u64 v = (u64)(((u128)j * P + ((u128)1 << E) - 1) >> E); x.push_back(v); x.push_back(v - 1); }
        for (int E = 33; E < 64; E++) { x.push_back(1ULL << (96 - E)); x.push_back(((1ULL << (E - 32)) - 1) << (96 - E)); }
        for (size_t i = 0; i < (1u << 14); i++) x.push_back(hac[164 * 164 + 12 + i]);
        check_all_shl(x, std::make_integer_sequence<int, 95>());
    }
    printf("failing functions: %d\n", g_failed);
    return g_failed > 255 ? 255 : g_failed;
}
