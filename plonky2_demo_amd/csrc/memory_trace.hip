// MemoryStark::generate_trace (evm/src/memory/memory_stark.rs:120-237) on the device: the 26 columns of evm's memory table from a log
// of memory operations, without a per-op serial pass.  gl_memory_trace_host (host_api.hip) is the reference's loops statement by
// statement; here they are restated:
//   - the stable sort by (context, segment, virt, timestamp) is two stable 64-bit passes of the library's radix sort that carry the index;
//   - fill_gaps pushes, per sorted neighbour pair, a number of rows that the pair alone fixes, and every pushed row's key lies strictly
//     between its pair's keys: the second sort is a merge at known places, a prefix sum over the counts;
//   - pad_memory_ops copies the last row pushed (or, if none was, the last op): the padding block stands directly behind that row;
//   - one thread per row of the trace finds its source by binary search over the places and looks at the next row for its flags;
//   - the permuted columns are gl_stark_lookup_columns' body (stark_lookup.hpp) on the one lookup (22, 23, 24, 25).
// gl_memory_trace_new waits for the stream once, for the height; gl_memory_trace_fill never does.
#include "stark_lookup.hpp"
#include "memory_trace_kernels.cuh"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <memory>

struct gl_memory_trace {
    gl_ctx* ctx = nullptr;
    uint32_t num_ops = 0, n = 0, merged = 0, last_place = 0, max_rc = 0;
    void* d_key = nullptr; void* d_kind = nullptr; void* d_value = nullptr; void* d_place = nullptr;      // blocks of the context's pool
    gllookup::Plan plan;                        // of the lookup (22, 23, 24, 25) at n rows; n == 1 has none
    void* d_words = nullptr;                    // plan.words in HBM
};

extern "C" void gl_memory_trace_free(gl_memory_trace* t) noexcept {
    if (!t) return;
    if (t->ctx) {
        for (void* p : {t->d_key, t->d_kind, t->d_value, t->d_place, t->d_words})
            if (p) t->ctx->pool_release(p);
        gl_ctx_release(t->ctx);
    }
    delete t;
}
extern "C" size_t gl_memory_trace_rows(const gl_memory_trace* t) noexcept { return t ? t->n : 0; }

namespace {
int memory_trace_new(gl_ctx* c, const gl_memory_op* ops, bool on_device, size_t num_ops_in, gl_memory_trace** out) {
    GL_REQUIRE(c && ops && out, GL_ERR_ARG, "gl_memory_trace_new: null argument");
    GL_REQUIRE(num_ops_in >= 1, GL_ERR_ARG, "gl_memory_trace_new: no memory ops");            // :195 expect("No memory ops?")
    GL_REQUIRE(num_ops_in <= (size_t(1) << GL_MEMORY_MAX_LOG_ROWS), GL_ERR_UNSUPPORTED, "gl_memory_trace_new: more than 2^24 rows");
    GL_TRY(c->activate());
    hipStream_t st = c->stream;
    GlTimed timed(c, "memory trace: sort and count");
    const uint32_t num_ops = (uint32_t)num_ops_in, blocks = (num_ops + 255) / 256, nseg = (num_ops + GLM_SEG - 1) / GLM_SEG;
    uint32_t lg_rc = 0;
    while ((size_t(1) << lg_rc) < num_ops_in) lg_rc++;
    const uint32_t max_rc = (1u << lg_rc) - 1u;                                             // :164, from the length before gap filling
    std::unique_ptr<gl_memory_trace, void (*)(gl_memory_trace*)> t(new gl_memory_trace(), gl_memory_trace_free);
    t->ctx = c; c->retain();
    t->num_ops = num_ops; t->max_rc = max_rc;
    GL_TRY(c->pool_alloc((size_t)num_ops * sizeof(uint4), &t->d_key));
    GL_TRY(c->pool_alloc((size_t)num_ops * sizeof(uint32_t), &t->d_kind));
    GL_TRY(c->pool_alloc((size_t)num_ops * 2 * sizeof(uint4), &t->d_value));
    GL_TRY(c->pool_alloc((size_t)num_ops * sizeof(uint32_t), &t->d_place));
    // from the log's upload to the one wait no return leaves work on the stream that reads the caller's memory
    struct Settle { hipStream_t st; bool pending = false; ~Settle() { if (pending) (void)gl_stream_wait(st); } } settle{st};
    DevBuf d_ops(c), d_keys(c), d_keys_out(c), d_idx(c), d_idx_out(c), d_count(c), d_seg(c), d_stats(c), d_tmp(c);
    if (!on_device) {
        GL_TRY(d_ops.alloc((size_t)num_ops * sizeof(gl_memory_op)));
        GL_CHECK_HIP(hipMemcpyAsync(d_ops.p, ops, (size_t)num_ops * sizeof(gl_memory_op), hipMemcpyHostToDevice, st));
        ops = d_ops.as<const gl_memory_op>();
    }
    settle.pending = true;
    GL_TRY(d_keys.alloc((size_t)num_ops * 8));
    GL_TRY(d_keys_out.alloc((size_t)num_ops * 8));
    GL_TRY(d_idx.alloc((size_t)num_ops * 4));
    GL_TRY(d_idx_out.alloc((size_t)num_ops * 4));
    GL_TRY(d_count.alloc((size_t)num_ops * 4));
    GL_TRY(d_seg.alloc((size_t)nseg * 4));
    GL_TRY(d_stats.alloc(sizeof(GlMemStats)));
    size_t tb = 0;
    GL_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, d_keys.as<const uint64_t>(), d_keys_out.as<uint64_t>(), d_idx.as<const uint32_t>(), d_idx_out.as<uint32_t>(),
                                                    (int)num_ops, 0, 64, st));
    GL_TRY(d_tmp.alloc(tb ? tb : 16));
    GL_CHECK_HIP(hipMemsetAsync(d_stats.p, 0, sizeof(GlMemStats), st));
    GlMemStats* stats = d_stats.as<GlMemStats>();
    // sort_by_key(MemoryOp::sorting_key) (:125): stable, by (virt, timestamp) and then by (context, segment)
    hipLaunchKernelGGL(k_mem_keys_low, dim3(blocks), dim3(256), 0, st, ops, num_ops, d_keys.as<uint64_t>(), d_idx.as<uint32_t>(), stats);
    GL_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tb, d_keys.as<const uint64_t>(), d_keys_out.as<uint64_t>(), d_idx.as<const uint32_t>(), d_idx_out.as<uint32_t>(),
                                                    (int)num_ops, 0, 64, st));
    hipLaunchKernelGGL(k_mem_keys_high, dim3(blocks), dim3(256), 0, st, ops, d_idx_out.as<const uint32_t>(), num_ops, d_keys.as<uint64_t>(), stats);
    GL_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tb, d_keys.as<const uint64_t>(), d_keys_out.as<uint64_t>(), d_idx_out.as<const uint32_t>(), d_idx.as<uint32_t>(),
                                                    (int)num_ops, 0, 64, st));
    hipLaunchKernelGGL(k_mem_gather, dim3(blocks), dim3(256), 0, st, ops, d_idx.as<const uint32_t>(), num_ops, (uint4*)t->d_key, (uint32_t*)t->d_kind, (uint4*)t->d_value, stats);
    // fill_gaps (:163-192) as counts, and where every op lands among the rows it pushes
    hipLaunchKernelGGL(k_mem_counts, dim3(blocks), dim3(256), 0, st, (const uint4*)t->d_key, num_ops, max_rc, lg_rc, d_count.as<uint32_t>(), stats);
    hipLaunchKernelGGL(k_mem_seg_sums, dim3(nseg), dim3(256), 0, st, d_count.as<const uint32_t>(), num_ops, d_seg.as<uint32_t>());
    hipLaunchKernelGGL(k_mem_seg_scan, dim3(1), dim3(64), 0, st, d_seg.as<uint32_t>(), nseg);
    hipLaunchKernelGGL(k_mem_positions, dim3(nseg), dim3(256), 0, st, d_count.as<const uint32_t>(), d_seg.as<const uint32_t>(), num_ops, (uint32_t*)t->d_place, stats);
    GL_CHECK_HIP(hipGetLastError());
    GlMemStats h{};
    GL_TRY(gl_copy_d2h(c, &h, d_stats.p, sizeof h));                                        // the one wait: the height
    settle.pending = false;
    GL_REQUIRE(!(h.bad_flags & 2u), GL_ERR_INTERNAL, "gl_memory_trace_new: a sort handed back an index outside the log");
    GL_REQUIRE(!h.bad_flags, GL_ERR_ARG, "gl_memory_trace_new: filter and is_read are 0 or 1");
    GL_REQUIRE(num_ops + h.pushed <= (uint64_t(1) << GL_MEMORY_MAX_LOG_ROWS), GL_ERR_UNSUPPORTED, "gl_memory_trace_new: more than 2^24 rows");
    const uint32_t merged = num_ops + (uint32_t)h.pushed;
    uint32_t n = 1;
    while (n < merged) n <<= 1;                                                             // pad_memory_ops (:207-208)
    GL_REQUIRE(h.max_step < n, GL_ERR_ARG, "gl_memory_trace_new: a range check is too large (a context or segment step of more than the trace's height)");
    t->merged = merged; t->n = n;
    t->last_place = h.last_pair ? h.last_place : merged - 1;
    GL_REQUIRE(t->last_place < merged, GL_ERR_INTERNAL, "gl_memory_trace_new: the last pushed row lies outside the merged trace");
    if (n >= 2) {
        const gl_stark_lookup lookup = {GL_MEMORY_RANGE_CHECK, GL_MEMORY_COUNTER, GL_MEMORY_RANGE_CHECK_PERMUTED, GL_MEMORY_COUNTER_PERMUTED};
        GL_TRY(gllookup::plan(GL_MEMORY_NUM_COLUMNS, n, &lookup, 1, &t->plan));
        GlMemWords words{};                     // by value through a launch: the handle may be freed at once, no host source is read later
        GL_REQUIRE(t->plan.words.size() <= GLM_MAX_WORDS, GL_ERR_INTERNAL, "gl_memory_trace_new: the lookup's plan has more words than expected");
        words.count = (uint32_t)t->plan.words.size();
        std::copy(t->plan.words.begin(), t->plan.words.end(), words.w);
        GL_TRY(c->pool_alloc(GLM_MAX_WORDS * 4, &t->d_words));
        hipLaunchKernelGGL(k_mem_words, dim3(1), dim3(64), 0, st, words, (uint32_t*)t->d_words);
        GL_CHECK_HIP(hipGetLastError());
    }
    *out = t.release();
    return GL_OK;
}
}  // namespace

extern "C" int gl_memory_trace_new(gl_ctx* c, const gl_memory_op* h_ops, size_t num_ops, gl_memory_trace** out) try {
    return memory_trace_new(c, h_ops, false, num_ops, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_memory_trace_new_device(gl_ctx* c, const gl_memory_op* d_ops, size_t num_ops, gl_memory_trace** out) try {
    return memory_trace_new(c, d_ops, true, num_ops, out);
} catch (...) { return gl_caught(); }

extern "C" int gl_memory_trace_fill(gl_memory_trace* t, uint64_t* d_cols) try {
    GL_REQUIRE(t && d_cols, GL_ERR_ARG, "gl_memory_trace_fill: null argument");
    gl_ctx* c = t->ctx;
    GL_TRY(c->activate());
    GlTimed timed(c, "memory trace: fill");
    GlMemSorted s;
    s.key = (const uint4*)t->d_key; s.kind = (const uint32_t*)t->d_kind; s.value = (const uint4*)t->d_value; s.place = (const uint32_t*)t->d_place;
    s.num_ops = t->num_ops; s.n = t->n; s.merged = t->merged; s.last_place = t->last_place; s.max_rc = t->max_rc;
    hipLaunchKernelGGL(k_mem_fill, dim3((t->n + 255) / 256), dim3(256), 0, c->stream, s, d_cols);
    GL_CHECK_HIP(hipGetLastError());
    if (t->n >= 2) {
        GlTimed lookup(c, "lookup columns");
        GL_TRY(gllookup::run(c, d_cols, t->plan, (const uint32_t*)t->d_words));
    }
    return GL_OK;
} catch (...) { return gl_caught(); }
