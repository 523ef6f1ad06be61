// Kernels of gl_stark_lookup_columns (stark_lookup.hip): permuted_cols (evm/src/lookup.rs:65-127) for many lookups of one trace.  Every
// kernel takes the lookup of a call's chunk from blockIdx.y, so a phase is one launch whatever the number of lookups.  DESIGN.md
// section 19 derives the formulation; the order of the phases is
//   k_lookup_canon                                          canonical keys of the source columns, for the library's 64-bit sort
//   k_lookup_classify                                       occurrence indices by binary search: the Equal case, the push / pop events
//   k_lookup_seg_sums / k_lookup_seg_scan / k_lookup_level_keys   stack levels: the prefix sum over the events in merge order -> sort keys
//   k_lookup_match                                          after the library's stable sort by level: matched pairs are neighbours
//   k_lookup_seg_sums / k_lookup_seg_scan / k_lookup_ranks  ranks of the leftover pops and pushes
//   k_lookup_left_values / k_lookup_left_fill               the k-th leftover position takes the k-th leftover value
#pragma once
#include "gl64.cuh"

#define GLK_SEG 2048            // elements per workgroup segment of a scan (256 threads x 8), the house size of stark_segments.cuh
#define GLK_NONE 0u             // event kinds, bits 31..30 of an event word; bits 29..0 = the position in its own sorted array
#define GLK_PUSH 1u
#define GLK_POP 2u              // a live pop
#define GLK_DEAD 3u             // a pop at or above the table's largest value: the loop has left (j == n), it is deferred
#define GLK_POS_MASK 0x3fffffffu

struct GlLookupDev { uint32_t a_slot, t_slot, col_permuted_input, col_permuted_table; };      // slots index the chunk's sorted columns

// number of elements of the ascending s[0..n) below v (lower) / not above v (upper); n a power of two: log2(n) + 1 probes, no branch
// on the data.  The probes of neighbouring threads fall on the same lines, and a column of 2^16 words is 512 KiB: they stay in L2.
__device__ __forceinline__ uint32_t lk_lower(const uint64_t* __restrict__ s, uint32_t n, uint64_t v) {
    uint32_t lo = 0;
    for (uint32_t step = n >> 1; step; step >>= 1) lo += (s[lo + step - 1] < v) ? step : 0u;
    return lo + (s[lo] < v ? 1u : 0u);
}
__device__ __forceinline__ uint32_t lk_upper(const uint64_t* __restrict__ s, uint32_t n, uint64_t v) {
    uint32_t lo = 0;
    for (uint32_t step = n >> 1; step; step >>= 1) lo += (s[lo + step - 1] <= v) ? step : 0u;
    return lo + (s[lo] <= v ? 1u : 0u);
}

// inclusive sum over the 64 lanes of a wave
__device__ __forceinline__ int lk_wave_inclusive(int v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= (uint32_t)d) v += o; }
    return v;
}
// exclusive sum of v over the 256 threads of a workgroup; *total = the sum of all of them.  sh: four words of LDS
__device__ __forceinline__ int lk_block_exclusive(int v, int* sh, int* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int inc = lk_wave_inclusive(v);
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    const int s0 = sh[0], s1 = sh[1], s2 = sh[2], s3 = sh[3];
    *total = s0 + s1 + s2 + s3;
    return inc - v + (wave > 0 ? s0 : 0) + (wave > 1 ? s1 : 0) + (wave > 2 ? s2 : 0);
}

// keys[slot][i] = the canonical word of source column slot_col[slot]
__global__ __launch_bounds__(256) void k_lookup_canon(const uint64_t* __restrict__ cols, uint32_t n, const uint32_t* __restrict__ slot_col, uint32_t slot0,
                                                      uint64_t* __restrict__ keys) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, slot = slot0 + blockIdx.y;
    if (i >= n) return;
    keys[(size_t)slot * n + i] = gl_canon(cols[(size_t)slot_col[slot] * n + i]);
}

// Element x < n is position i = x of the sorted inputs a, element x >= n position j = x - n of the sorted table t.  occ = the position
// among the equal values of its own array; an input with occ < cnt_t(value) is the Equal case of the loop and takes its own value, any
// other input is a pop; a table position with occ >= cnt_a(value) is a push.  Every element goes to its place m of the merge of the two
// arrays (inputs before equal table values; no value has events of both kinds, so the order of events is the loop's): w[m] = +1 push,
// -1 live pop, 0 otherwise; ev[m] = kind << 30 | own position.  flag[x] = 1 for a dead pop (k_lookup_match adds the unmatched events).
// Also writes the permuted input column.
__global__ __launch_bounds__(256) void k_lookup_classify(const uint64_t* __restrict__ sorted, const GlLookupDev* __restrict__ lk, uint32_t n,
                                                         uint64_t* __restrict__ cols, int* __restrict__ w, uint32_t* __restrict__ ev, uint32_t* __restrict__ flag) {
    const uint32_t x = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (x >= 2 * n) return;
    const GlLookupDev d = lk[l];
    const uint64_t* a = sorted + (size_t)d.a_slot * n;
    const uint64_t* t = sorted + (size_t)d.t_slot * n;
    const size_t base = (size_t)l * 2 * n;
    if (x < n) {
        const uint64_t v = a[x];
        const uint32_t occ = x - lk_lower(a, n, v), lo = lk_lower(t, n, v), cnt_t = lk_upper(t, n, v) - lo;
        uint32_t kind = GLK_NONE;
        if (occ < cnt_t) cols[(size_t)d.col_permuted_table * n + x] = v;
        else kind = (v >= t[n - 1]) ? GLK_DEAD : GLK_POP;
        cols[(size_t)d.col_permuted_input * n + x] = v;
        const uint32_t m = x + lo;                                  // the table values below v stand before it
        w[base + m] = (kind == GLK_POP) ? -1 : 0;
        ev[base + m] = kind << 30 | x;
        flag[base + x] = (kind == GLK_DEAD) ? 1u : 0u;
    } else {
        const uint32_t j = x - n;
        const uint64_t v = t[j];
        const uint32_t occ = j - lk_lower(t, n, v), lo = lk_lower(a, n, v), up = lk_upper(a, n, v);
        const uint32_t kind = (occ >= up - lo) ? GLK_PUSH : GLK_NONE;
        const uint32_t m = j + up;                                  // the inputs not above v stand before it
        w[base + m] = (kind == GLK_PUSH) ? 1 : 0;
        ev[base + m] = kind << 30 | j;
        flag[base + x] = 0u;
    }
}

// ---- exclusive additive scan over src[lookup][len] in the house shape: segment sums, a scan of the segment sums, a finalize ----
__global__ __launch_bounds__(256) void k_lookup_seg_sums(const int* __restrict__ src, uint32_t len, int* __restrict__ seg_sum) {
    __shared__ int sh[4];
    const uint32_t l = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
    const int* rp = src + (size_t)l * len;
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLK_SEG + t * 8 + q; if (i < len) acc += rp[i]; }
    int total;
    (void)lk_block_exclusive(acc, sh, &total);
    if (t == 0) seg_sum[(size_t)l * gridDim.x + seg] = total;
}
// one wave per lookup walks its segment sums 64 at a time: seg_sum becomes the exclusive prefix
__global__ __launch_bounds__(64) void k_lookup_seg_scan(int* __restrict__ seg_sum, uint32_t nseg) {
    int* rp = seg_sum + (size_t)blockIdx.x * nseg;
    const uint32_t lane = threadIdx.x;
    int carry = 0;
    for (uint32_t s0 = 0; s0 < nseg; s0 += 64) {
        const uint32_t s = s0 + lane;
        const int v = s < nseg ? rp[s] : 0;
        const int inc = lk_wave_inclusive(v);
        if (s < nseg) rp[s] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
}
// finalize of the level scan: s = the sum of w before merge position m.  A push stands on level s + 1, a live pop on level s; the sort
// key is lookup << level_bits | level + n (levels lie in [-n, n]), and everything else gets the key behind the last lookup's.
__global__ __launch_bounds__(256) void k_lookup_level_keys(const int* __restrict__ w, const uint32_t* __restrict__ ev, const int* __restrict__ seg_excl, uint32_t n,
                                                           uint32_t level_bits, uint32_t num_lookups, uint32_t* __restrict__ keys) {
    __shared__ int sh[4];
    const uint32_t l = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, len = 2 * n;
    const size_t base = (size_t)l * len;
    int loc[8];
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLK_SEG + t * 8 + q; loc[q] = acc; if (i < len) acc += w[base + i]; }
    int total;
    const int prefix = seg_excl[(size_t)l * gridDim.x + seg] + lk_block_exclusive(acc, sh, &total);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint32_t i = seg * GLK_SEG + t * 8 + q;
        if (i < len) {
            const uint32_t kind = ev[base + i] >> 30;
            const int s = prefix + loc[q];
            uint32_t key = num_lookups << level_bits;
            if (kind == GLK_PUSH) key = l << level_bits | (uint32_t)(s + 1 + (int)n);
            else if (kind == GLK_POP) key = l << level_bits | (uint32_t)(s + (int)n);
            keys[base + i] = key;
        }
    }
}
// finalize of the leftover scan: rank[x] = the number of flagged elements before x
__global__ __launch_bounds__(256) void k_lookup_ranks(const int* __restrict__ flag, const int* __restrict__ seg_excl, uint32_t len, int* __restrict__ rank) {
    __shared__ int sh[4];
    const uint32_t l = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)l * len;
    int loc[8];
    int acc = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLK_SEG + t * 8 + q; loc[q] = acc; if (i < len) acc += flag[base + i]; }
    int total;
    const int prefix = seg_excl[(size_t)l * gridDim.x + seg] + lk_block_exclusive(acc, sh, &total);
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLK_SEG + t * 8 + q; if (i < len) rank[base + i] = prefix + loc[q]; }
}

// The events stably sorted by (lookup, level): a push and the pop that takes it are neighbours (a level's events alternate, and the
// pop that follows a push on its level is the one that finds it on top of the stack).  A matched pop takes the push's table value;
// an unmatched event is flagged a leftover.
__global__ __launch_bounds__(256) void k_lookup_match(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t total, uint32_t level_bits,
                                                      uint32_t num_lookups, uint32_t n, const GlLookupDev* __restrict__ lk, const uint64_t* __restrict__ sorted,
                                                      uint64_t* __restrict__ cols, uint32_t* __restrict__ flag) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    const uint32_t key = keys[k], l = key >> level_bits;
    if (l >= num_lookups) return;
    const uint32_t val = vals[k], kind = val >> 30, pos = val & GLK_POS_MASK;
    if (pos >= n) return;
    const GlLookupDev d = lk[l];
    if (kind == GLK_POP) {
        const uint32_t before = k ? vals[k - 1] : 0u;
        if (k && keys[k - 1] == key && (before >> 30) == GLK_PUSH && (before & GLK_POS_MASK) < n)
            cols[(size_t)d.col_permuted_table * n + pos] = sorted[(size_t)d.t_slot * n + (before & GLK_POS_MASK)];
        else flag[(size_t)l * 2 * n + pos] = 1u;
    } else if (kind == GLK_PUSH) {
        if (!(k + 1 < total && keys[k + 1] == key && (vals[k + 1] >> 30) == GLK_POP)) flag[(size_t)l * 2 * n + n + pos] = 1u;
    }
}

// left[lookup][k] = the k-th leftover table value in ascending table position (the stack from the bottom, then sorted_table[j..n))
__global__ __launch_bounds__(256) void k_lookup_left_values(const uint32_t* __restrict__ flag, const int* __restrict__ rank, const GlLookupDev* __restrict__ lk,
                                                            const uint64_t* __restrict__ sorted, uint32_t n, uint64_t* __restrict__ left) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (j >= n) return;
    const size_t base = (size_t)l * 2 * n;
    if (!flag[base + n + j]) return;
    const uint32_t k = (uint32_t)(rank[base + n + j] - rank[base + n]);
    if (k < n) left[(size_t)l * n + k] = sorted[(size_t)lk[l].t_slot * n + j];
}
// ... and the k-th leftover input position (ascending: the deferred pops, then the dead ones) takes it
__global__ __launch_bounds__(256) void k_lookup_left_fill(const uint32_t* __restrict__ flag, const int* __restrict__ rank, const GlLookupDev* __restrict__ lk,
                                                          const uint64_t* __restrict__ left, uint32_t n, uint64_t* __restrict__ cols) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (i >= n) return;
    const size_t base = (size_t)l * 2 * n;
    if (!flag[base + i]) return;
    const uint32_t k = (uint32_t)rank[base + i];
    if (k < n) cols[(size_t)lk[l].col_permuted_table * n + i] = left[(size_t)l * n + k];
}
