// Kernels of gl_memory_trace_new / gl_memory_trace_fill (memory_trace.hip): MemoryStark::generate_trace (evm/src/memory/memory_stark.rs:
// 120-237) without its loops.  DESIGN.md section 20 derives the formulation; the order of the launches is
//   k_mem_keys_low / k_mem_keys_high          the keys of the two stable 64-bit sorts (the library's radix sort): (virt, timestamp), then
//                                             (context, segment), carrying the op's index; the first also looks at filter and is_read
//   k_mem_gather                              the ops in sorted order: key, kind and value apart, so that a row's loads are whole lines
//   k_mem_counts                              per sorted neighbour pair the rows fill_gaps pushes for it; their sum, the largest context /
//                                             segment step and the last pair that pushes anything go to the statistics the host reads
//   k_mem_seg_sums / k_mem_seg_scan / k_mem_positions   the prefix sum over the counts: sorted op i stands on merged place i + sum before i
//   k_mem_words                               the few words of the lookup's plan, passed by value: no host buffer has to outlive a copy
//   k_mem_fill                                one thread per row of the trace: its source by binary search over the places, the next
//                                             row's key the same way, 24 coalesced column stores (26 for a trace of one row)
#pragma once
#include "gl64.cuh"
#include "../../include/plonky2_mi355x.h"

#define GLM_SEG 2048            // elements per workgroup segment of the scan (256 threads x 8), the house size of stark_segments.cuh
#define GLM_COUNT_CAP (1u << 25)      // a pair's count as the scan sees it: above the largest trace, so a log that fits is never clamped

struct GlMemStats {             // what gl_memory_trace_new reads back, once
    unsigned long long pushed;  // rows fill_gaps pushes, over all pairs, in 64 bits: one pair can ask for 2^31
    uint32_t max_step;          // the largest (context or segment step) - 1 between sorted neighbours: the assertion of :112-116
    uint32_t bad_flags;         // bit 0: an op's filter or is_read is neither 0 nor 1; bit 1: a sort handed back an index >= num_ops
    uint32_t last_pair;         // 1 + the last sorted pair that pushes a row (0: none does): pad_memory_ops copies its last dummy
    uint32_t last_place;        // the merged place of that dummy (k_mem_positions writes it where last_pair != 0)
};
#define GLM_MAX_WORDS 16u
struct GlMemWords { uint32_t count; uint32_t w[GLM_MAX_WORDS]; };      // a kernel argument
struct GlMemSorted {            // the sorted log as k_mem_gather leaves it
    const uint4* key;           // (context, segment, virt, timestamp)
    const uint32_t* kind;       // filter | is_read << 1
    const uint4* value;         // [num_ops][2]: the eight limbs
    const uint32_t* place;      // sorted op i stands on merged place place[i] = i + the rows pushed for the pairs before it
    uint32_t num_ops, n;        // n: the trace's height
    uint32_t merged;            // num_ops + the rows pushed: the trace before pad_memory_ops
    uint32_t last_place;        // the merged place of memory_ops.last() after fill_gaps: the padding block stands behind it
    uint32_t max_rc;            // next_power_of_two(num_ops) - 1
};

__device__ __forceinline__ uint32_t mem_wave_inclusive(uint32_t v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= (uint32_t)d) v += o; }
    return v;
}
// exclusive sum of v over the 256 threads of a workgroup; *total = the sum of all of them.  sh: four words of LDS
__device__ __forceinline__ uint32_t mem_block_exclusive(uint32_t v, uint32_t* sh, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = mem_wave_inclusive(v);
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    const uint32_t s0 = sh[0], s1 = sh[1], s2 = sh[2], s3 = sh[3];
    *total = s0 + s1 + s2 + s3;
    return inc - v + (wave > 0 ? s0 : 0u) + (wave > 1 ? s1 : 0u) + (wave > 2 ? s2 : 0u);
}

// keys[i] = virt << 32 | timestamp, idx[i] = i: the first of the two stable passes sorts by the key's low half
__global__ __launch_bounds__(256) void k_mem_keys_low(const gl_memory_op* __restrict__ ops, uint32_t num_ops, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                      GlMemStats* __restrict__ stats) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_ops) return;
    const gl_memory_op op = ops[i];
    keys[i] = (uint64_t)op.virt << 32 | op.timestamp;
    idx[i] = i;
    if (op.filter > 1u || op.is_read > 1u) atomicOr(&stats->bad_flags, 1u);
}
// keys[k] = context << 32 | segment of the op that stands on place k after the first pass
__global__ __launch_bounds__(256) void k_mem_keys_high(const gl_memory_op* __restrict__ ops, const uint32_t* __restrict__ idx, uint32_t num_ops,
                                                       uint64_t* __restrict__ keys, GlMemStats* __restrict__ stats) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= num_ops) return;
    const uint32_t i = idx[k];
    if (i >= num_ops) { atomicOr(&stats->bad_flags, 2u); keys[k] = ~0ull; return; }      // never with a correct sort: gl_memory_trace_new refuses
    keys[k] = (uint64_t)ops[i].context << 32 | ops[i].segment;
}
__global__ __launch_bounds__(256) void k_mem_gather(const gl_memory_op* __restrict__ ops, const uint32_t* __restrict__ idx, uint32_t num_ops, uint4* __restrict__ key,
                                                    uint32_t* __restrict__ kind, uint4* __restrict__ value, GlMemStats* __restrict__ stats) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= num_ops) return;
    uint32_t i = idx[k];
    if (i >= num_ops) { atomicOr(&stats->bad_flags, 2u); i = 0; }                        // as above; every word is still written
    const gl_memory_op op = ops[i];
    key[k] = make_uint4(op.context, op.segment, op.virt, op.timestamp);
    kind[k] = (op.filter & 1u) | (op.is_read & 1u) << 1;
    value[2 * (size_t)k] = make_uint4(op.value[0], op.value[1], op.value[2], op.value[3]);
    value[2 * (size_t)k + 1] = make_uint4(op.value[4], op.value[5], op.value[6], op.value[7]);
}

// fill_gaps (:163-192) counted, not run: pair (i, i + 1) with equal context and segment pushes (virt gap) >> log2(max_rc + 1) reads at a
// new virt, or with an equal address ceil(timestamp step / max_rc) - 1 at a new timestamp.  count[num_ops - 1] = 0.
__global__ __launch_bounds__(256) void k_mem_counts(const uint4* __restrict__ key, uint32_t num_ops, uint32_t max_rc, uint32_t lg_rc, uint32_t* __restrict__ count,
                                                    GlMemStats* __restrict__ stats) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long c = 0;
    uint32_t step = 0;
    if (i + 1 < num_ops) {
        const uint4 a = key[i], b = key[i + 1];
        if (a.x != b.x) step = b.x - a.x - 1u;
        else if (a.y != b.y) step = b.y - a.y - 1u;
        else if (a.z != b.z) c = (unsigned long long)(b.z - a.z - 1u) >> lg_rc;
        else if (a.w != b.w) c = (unsigned long long)(b.w - a.w - 1u) / max_rc;      // max_rc >= 1 where there is a pair
    }
    if (i < num_ops) count[i] = c > GLM_COUNT_CAP ? GLM_COUNT_CAP : (uint32_t)c;
    uint32_t last = c ? i + 1u : 0u;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        c += __shfl_xor(c, d, 64);
        step = max(step, (uint32_t)__shfl_xor(step, d, 64));
        last = max(last, (uint32_t)__shfl_xor(last, d, 64));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (c) atomicAdd(&stats->pushed, c);
        if (step) atomicMax(&stats->max_step, step);
        if (last) atomicMax(&stats->last_pair, last);
    }
}

// ---- exclusive additive scan over count[num_ops] in the house shape: segment sums, a scan of the segment sums, a finalize ----
__global__ __launch_bounds__(256) void k_mem_seg_sums(const uint32_t* __restrict__ src, uint32_t len, uint32_t* __restrict__ seg_sum) {
    __shared__ uint32_t sh[4];
    const uint32_t seg = blockIdx.x, t = threadIdx.x;
    uint32_t acc = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLM_SEG + t * 8 + q; if (i < len) acc += src[i]; }
    uint32_t total;
    (void)mem_block_exclusive(acc, sh, &total);
    if (t == 0) seg_sum[seg] = total;
}
// one wave walks the segment sums 64 at a time: seg_sum becomes the exclusive prefix
__global__ __launch_bounds__(64) void k_mem_seg_scan(uint32_t* __restrict__ seg_sum, uint32_t nseg) {
    const uint32_t lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t s0 = 0; s0 < nseg; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t v = s < nseg ? seg_sum[s] : 0u;
        const uint32_t inc = mem_wave_inclusive(v);
        if (s < nseg) seg_sum[s] = carry + inc - v;
        carry += __shfl(inc, 63, 64);
    }
}
// place[i] = i + the sum of count before i; the last pushed row stands just before the op behind its pair
__global__ __launch_bounds__(256) void k_mem_positions(const uint32_t* __restrict__ count, const uint32_t* __restrict__ seg_excl, uint32_t len,
                                                       uint32_t* __restrict__ place, GlMemStats* stats) {
    __shared__ uint32_t sh[4];
    const uint32_t seg = blockIdx.x, t = threadIdx.x;
    uint32_t loc[8];
    uint32_t acc = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLM_SEG + t * 8 + q; loc[q] = acc; if (i < len) acc += count[i]; }
    uint32_t total;
    const uint32_t prefix = seg_excl[seg] + mem_block_exclusive(acc, sh, &total);
    const uint32_t last_pair = stats->last_pair;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint32_t i = seg * GLM_SEG + t * 8 + q;
        if (i < len) {
            place[i] = i + prefix + loc[q];
            if (i && i == last_pair) stats->last_place = i + prefix + loc[q] - 1u;
        }
    }
}

// out[i] = p.w[i]: the selection is unrolled, so the argument's array is never indexed at run time
__global__ __launch_bounds__(64) void k_mem_words(GlMemWords p, uint32_t* __restrict__ out) {
    const uint32_t i = threadIdx.x;
    if (i >= p.count) return;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < GLM_MAX_WORDS; k++) v = (i == k) ? p.w[k] : v;
    out[i] = v;
}

// Row r of the trace after the second sort: the merged list of ops and pushed rows with the padding block, n - merged copies of the
// last pushed row (or of the last op), directly behind that row.  -> the sorted op i it comes from, j = 0 for the op itself or the
// number of the pushed row of pair (i, i + 1), whether it is a padding copy, and its key.
__device__ __forceinline__ void mem_row(const GlMemSorted& s, uint32_t r, uint32_t* op, uint32_t* j, bool* padding, bool* zero_value, uint4* key) {
    const uint32_t pad_rows = s.n - s.merged;
    uint32_t m = r;
    *padding = false;
    if (r > s.last_place) {
        *padding = r <= s.last_place + pad_rows;
        m = *padding ? s.last_place : r - pad_rows;
    }
    uint32_t lo = 0, hi = s.num_ops;                                  // place[lo] <= m < place[hi]; place[0] = 0
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s.place[mid] <= m) lo = mid; else hi = mid;
    }
    const uint32_t k = m - s.place[lo];
    uint4 a = s.key[lo];
    *zero_value = false;
    if (k && lo + 1u < s.num_ops) {
        if (s.key[lo + 1].z != a.z) { a.z += k * (s.max_rc + 1u); a.w = 0u; *zero_value = true; }      // new_dummy_read(dummy_address, 0, U256::zero())
        else a.w += k * s.max_rc;                                                                       // new_dummy_read(curr.address, curr.timestamp + max_rc, curr.value)
    }
    *op = lo; *j = k; *key = a;
}

// into_row (:52-70), generate_first_change_flags_and_rc (:73-118) and COUNTER (:145) for row r; the permuted columns are the lookup's,
// except in a trace of one row, which has no lookup launches: there they are the zeros permuted_cols gives
__global__ __launch_bounds__(256) void k_mem_fill(GlMemSorted s, uint64_t* __restrict__ cols) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= s.n) return;
    const size_t n = s.n;
    uint32_t op, j;
    bool padding, zero_value;
    uint4 a;
    mem_row(s, r, &op, &j, &padding, &zero_value, &a);
    const bool own = j == 0u && !padding;                            // the op as the log has it; every other row is a read with filter 0
    const uint32_t kind = s.kind[op];
    uint4 v0 = make_uint4(0u, 0u, 0u, 0u), v1 = v0;
    if (!zero_value) { v0 = s.value[2 * (size_t)op]; v1 = s.value[2 * (size_t)op + 1]; }
    uint32_t cfc = 0, sfc = 0, vfc = 0;
    uint64_t rc = 0;
    if (r + 1u < s.n) {
        uint32_t op1, j1;
        bool p1, z1;
        uint4 b;
        mem_row(s, r + 1u, &op1, &j1, &p1, &z1, &b);
        cfc = a.x != b.x;
        sfc = !cfc && a.y != b.y;
        vfc = !cfc && !sfc && a.z != b.z;
        rc = cfc ? (uint64_t)b.x - a.x - 1u : sfc ? (uint64_t)b.y - a.y - 1u : vfc ? (uint64_t)b.z - a.z - 1u : (uint64_t)b.w - a.w;
    }
    cols[GL_MEMORY_FILTER * n + r] = own ? (kind & 1u) : 0u;
    cols[GL_MEMORY_TIMESTAMP * n + r] = a.w;
    cols[GL_MEMORY_IS_READ * n + r] = own ? (kind >> 1) : 1u;
    cols[GL_MEMORY_ADDR_CONTEXT * n + r] = a.x;
    cols[GL_MEMORY_ADDR_SEGMENT * n + r] = a.y;
    cols[GL_MEMORY_ADDR_VIRTUAL * n + r] = a.z;
    cols[(GL_MEMORY_VALUE_START + 0) * n + r] = v0.x;
    cols[(GL_MEMORY_VALUE_START + 1) * n + r] = v0.y;
    cols[(GL_MEMORY_VALUE_START + 2) * n + r] = v0.z;
    cols[(GL_MEMORY_VALUE_START + 3) * n + r] = v0.w;
    cols[(GL_MEMORY_VALUE_START + 4) * n + r] = v1.x;
    cols[(GL_MEMORY_VALUE_START + 5) * n + r] = v1.y;
    cols[(GL_MEMORY_VALUE_START + 6) * n + r] = v1.z;
    cols[(GL_MEMORY_VALUE_START + 7) * n + r] = v1.w;
    cols[GL_MEMORY_CONTEXT_FIRST_CHANGE * n + r] = cfc;
    cols[GL_MEMORY_SEGMENT_FIRST_CHANGE * n + r] = sfc;
    cols[GL_MEMORY_VIRTUAL_FIRST_CHANGE * n + r] = vfc;
#pragma unroll
    for (uint32_t c = GL_MEMORY_VIRTUAL_FIRST_CHANGE + 1; c < GL_MEMORY_RANGE_CHECK; c++) cols[c * n + r] = 0u;
    cols[GL_MEMORY_RANGE_CHECK * n + r] = rc;
    cols[GL_MEMORY_COUNTER * n + r] = r;
    if (s.n == 1u) { cols[GL_MEMORY_RANGE_CHECK_PERMUTED * n + r] = 0u; cols[GL_MEMORY_COUNTER_PERMUTED * n + r] = 0u; }
}
