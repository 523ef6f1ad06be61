// permuted_cols (evm/src/lookup.rs:65-127) on the device: the permuted input and permuted table columns of the Halo2-style lookup, for
// every lookup of a trace in one call and in place (ArithmeticStark::generate_range_checks, arithmetic_stark.rs:97-118, calls it once
// per shared column against one RANGE_COUNTER column; MemoryStark once, memory_stark.rs:148).
//
// The reference sorts both columns and fills the permuted table by a sequential merge with a LIFO stack of unused table values.  Here
// the sorts are the library's radix sort, and the merge is restated without its loop: occurrence indices by
// binary search give the Equal case and the push / pop events; a prefix sum over the events in merge order gives every event its stack
// level; a stable sort by level puts a push beside the pop that takes it; what stays unmatched is handed out in order by two ranks.
// Word for word the loop's result, for invalid lookups too.
//
// Lookups are worked in chunks of at most 2^23 / n (at least one): the temporaries of a chunk are bounded, and every phase of a chunk
// is ONE launch over its lookups.  A source column that several lookups of a chunk share is sorted once; one that stands in the same
// slot of the next chunk (a shared table does: tables take the first slots) is not sorted again.
#include "stark_lookup.hpp"
#include "stark_lookup_kernels.cuh"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdlib>
#include <cstring>

#define GLK_MAX_LOOKUPS 1024u
#define GLK_MAX_LOG_N 24u
#define GLK_CHUNK_ELEMS (size_t(1) << 23)      // lookups x n per chunk: about 80 bytes of temporaries per element

namespace {
using gllookup::Chunk;
// the sorts of slots [first, first + count): one segmented sort, or a loop of whole-array sorts (DESIGN.md section 19 has both times)
int sort_slots(bool segmented, void* d_tmp, size_t& tmp_bytes, const uint64_t* in, uint64_t* out, uint32_t n, uint32_t first, uint32_t count,
               const uint32_t* d_seg_offsets, hipStream_t st) {
    if (segmented) {
        GL_CHECK_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(d_tmp, tmp_bytes, in + (size_t)first * n, out + (size_t)first * n, (int)((size_t)count * n), (int)count,
                                                                d_seg_offsets, d_seg_offsets + 1, 0, 64, st));
        return GL_OK;
    }
    if (!d_tmp) {
        GL_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, in, out, (int)n, 0, 64, st));
        return GL_OK;
    }
    for (uint32_t s = first; s < first + count; s++)
        GL_CHECK_HIP(hipcub::DeviceRadixSort::SortKeys(d_tmp, tmp_bytes, in + (size_t)s * n, out + (size_t)s * n, (int)n, 0, 64, st));
    return GL_OK;
}
}  // namespace

// the call's rules and its plan: chunks, and per chunk its lookups with their slots, the slots' columns and the segment offsets of the sort
int gllookup::plan(uint32_t num_columns, size_t n_rows, const gl_stark_lookup* lookups, uint32_t count, Plan* out) {
    GL_REQUIRE(lookups && out, GL_ERR_ARG, "gl_stark_lookup_columns: null argument");
    GL_REQUIRE(count >= 1 && count <= GLK_MAX_LOOKUPS, GL_ERR_ARG, "gl_stark_lookup_columns: 1..1024 lookups");
    GL_REQUIRE(n_rows >= 2 && n_rows <= (size_t(1) << GLK_MAX_LOG_N) && (n_rows & (n_rows - 1)) == 0, GL_ERR_ARG,
               "gl_stark_lookup_columns: n is a power of two, 2..2^24");
    const uint32_t n = (uint32_t)n_rows;
    std::vector<uint32_t> sources, outputs;
    for (uint32_t l = 0; l < count; l++) {
        const gl_stark_lookup& k = lookups[l];
        GL_REQUIRE(k.col_input < num_columns && k.col_table < num_columns && k.col_permuted_input < num_columns && k.col_permuted_table < num_columns, GL_ERR_ARG,
                   "gl_stark_lookup_columns: column index out of range");
        sources.push_back(k.col_input); sources.push_back(k.col_table);
        outputs.push_back(k.col_permuted_input); outputs.push_back(k.col_permuted_table);
    }
    std::sort(sources.begin(), sources.end());
    std::sort(outputs.begin(), outputs.end());
    GL_REQUIRE(std::adjacent_find(outputs.begin(), outputs.end()) == outputs.end(), GL_ERR_ARG, "gl_stark_lookup_columns: two outputs share a column");
    for (uint32_t o : outputs)
        GL_REQUIRE(!std::binary_search(sources.begin(), sources.end(), o), GL_ERR_ARG, "gl_stark_lookup_columns: an output column is also an input or table column");
    uint32_t lg_n = 0;
    while ((size_t(1) << lg_n) < n_rows) lg_n++;
    const uint32_t per_chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(count, GLK_CHUNK_ELEMS / n_rows));
    std::vector<Chunk>& chunks = out->chunks;
    std::vector<uint32_t>& words = out->words;                      // every chunk's tables, uploaded once
    chunks.clear(); words.clear();
    std::vector<uint32_t> prev_slots;
    uint32_t max_slots = 0;
    for (uint32_t first = 0; first < count; first += per_chunk) {
        Chunk ch{};
        ch.first = first;
        ch.count = std::min(per_chunk, count - first);
        std::vector<uint32_t> slots;                                // slot -> source column: the tables in order of appearance, then the inputs
        auto slot_of = [&](uint32_t col) {
            const auto it = std::find(slots.begin(), slots.end(), col);
            if (it != slots.end()) return (uint32_t)(it - slots.begin());
            slots.push_back(col);
            return (uint32_t)slots.size() - 1;
        };
        std::vector<uint32_t> t_slot(ch.count), a_slot(ch.count);
        for (uint32_t l = 0; l < ch.count; l++) t_slot[l] = slot_of(lookups[first + l].col_table);
        for (uint32_t l = 0; l < ch.count; l++) a_slot[l] = slot_of(lookups[first + l].col_input);
        ch.num_slots = (uint32_t)slots.size();
        while (ch.keep < ch.num_slots && ch.keep < prev_slots.size() && prev_slots[ch.keep] == slots[ch.keep]) ch.keep++;
        ch.lk_off = words.size();
        for (uint32_t l = 0; l < ch.count; l++) {
            words.push_back(a_slot[l]); words.push_back(t_slot[l]);
            words.push_back(lookups[first + l].col_permuted_input); words.push_back(lookups[first + l].col_permuted_table);
        }
        ch.slot_off = words.size();
        words.insert(words.end(), slots.begin(), slots.end());
        ch.seg_off = words.size();
        for (uint32_t s = 0; s <= ch.num_slots - ch.keep; s++) words.push_back(s * n);      // at most 2 x 2^23 elements: 32 bits hold it
        max_slots = std::max(max_slots, ch.num_slots);
        prev_slots = slots;
        chunks.push_back(ch);
    }
    out->n = n; out->lg_n = lg_n; out->count = count; out->per_chunk = per_chunk; out->max_slots = max_slots;
    return GL_OK;
}

// Every launch of the call on the context's stream, its tables already in HBM (d_words: plan.words); temporaries from the pool.  Nothing
// here waits for the stream.
int gllookup::run(gl_ctx* c, uint64_t* d_cols, const Plan& plan, const uint32_t* d_words) {
    hipStream_t st = c->stream;
    const uint32_t n = plan.n, lg_n = plan.lg_n, per_chunk = plan.per_chunk, max_slots = plan.max_slots;
    const size_t n_rows = n;
    const std::vector<Chunk>& chunks = plan.chunks;
    const uint32_t level_bits = lg_n + 2;                           // levels + n lie in [0, 2n]
    // One segmented sort works a segment per workgroup: 2.1 ms flat at n = 2^16 whatever the number of columns, where a whole-array sort
    // costs 0.056 ms per column.  It pays from about 48 columns of 2^16 on, from fewer at smaller n.
    static const int sort_env = [] { const char* e = getenv("GL_LOOKUP_SEGMENTED_SORT"); return e ? atoi(e) : -1; }();      // tuning knob: 0 loop, 1 segmented
    const auto segmented = [&](uint32_t fresh) { return sort_env >= 0 ? sort_env != 0 : (lg_n <= 16 && fresh >= 2 && ((size_t)fresh << 16) >= 48 * n_rows); };

    // ---- temporaries from the pool ----
    const size_t chunk_elems = (size_t)per_chunk * 2 * n;           // merge positions of a chunk
    const uint32_t nseg = (2 * n + GLK_SEG - 1) / GLK_SEG;
    DevBuf d_canon(c), d_sorted(c), d_w(c), d_ev(c), d_flag(c), d_keys(c), d_keys_out(c), d_vals_out(c), d_seg(c), d_tmp(c);
    GL_TRY(d_canon.alloc((size_t)std::max(max_slots, per_chunk) * n * 8));      // the unsorted keys [slots][n]; afterwards the leftover values [lookups][n]
    GL_TRY(d_sorted.alloc((size_t)max_slots * n * 8));
    GL_TRY(d_w.alloc(chunk_elems * 4));                             // the events' weights; afterwards the leftover ranks
    GL_TRY(d_ev.alloc(chunk_elems * 4));
    GL_TRY(d_flag.alloc(chunk_elems * 4));
    GL_TRY(d_keys.alloc(chunk_elems * 4));
    GL_TRY(d_keys_out.alloc(chunk_elems * 4));
    GL_TRY(d_vals_out.alloc(chunk_elems * 4));
    GL_TRY(d_seg.alloc((size_t)per_chunk * nseg * 4));
    size_t tb_max = 16;                                             // the library's scratch: the largest any sort of any chunk asks for
    for (const Chunk& ch : chunks) {
        size_t tb_cols = 0, tb_events = 0;
        if (ch.num_slots > ch.keep)
            GL_TRY(sort_slots(segmented(ch.num_slots - ch.keep), nullptr, tb_cols, d_canon.as<uint64_t>(), d_sorted.as<uint64_t>(), n, ch.keep, ch.num_slots - ch.keep, d_words, st));
        GL_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_events, d_keys.as<const uint32_t>(), d_keys_out.as<uint32_t>(), d_ev.as<const uint32_t>(),
                                                        d_vals_out.as<uint32_t>(), (int)(ch.count * 2 * n), 0, (int)(level_bits + 32u - (uint32_t)__builtin_clz(ch.count)), st));
        tb_max = std::max(tb_max, std::max(tb_cols, tb_events));
    }
    GL_TRY(d_tmp.alloc(tb_max));

    for (const Chunk& ch : chunks) {
        const GlLookupDev* lk = (const GlLookupDev*)(d_words + ch.lk_off);
        const uint32_t* slot_col = d_words + ch.slot_off;
        const uint32_t fresh = ch.num_slots - ch.keep, total = ch.count * 2 * n;
        if (fresh) {
            hipLaunchKernelGGL(k_lookup_canon, dim3((n + 255) / 256, fresh), dim3(256), 0, st, (const uint64_t*)d_cols, n, slot_col, ch.keep, d_canon.as<uint64_t>());
            size_t tb = tb_max;
            GL_TRY(sort_slots(segmented(fresh), d_tmp.p, tb, d_canon.as<uint64_t>(), d_sorted.as<uint64_t>(), n, ch.keep, fresh, d_words + ch.seg_off, st));
        }
        hipLaunchKernelGGL(k_lookup_classify, dim3((2 * n + 255) / 256, ch.count), dim3(256), 0, st, d_sorted.as<const uint64_t>(), lk, n, d_cols, d_w.as<int>(),
                           d_ev.as<uint32_t>(), d_flag.as<uint32_t>());
        hipLaunchKernelGGL(k_lookup_seg_sums, dim3(nseg, ch.count), dim3(256), 0, st, d_w.as<const int>(), 2 * n, d_seg.as<int>());
        hipLaunchKernelGGL(k_lookup_seg_scan, dim3(ch.count), dim3(64), 0, st, d_seg.as<int>(), nseg);
        hipLaunchKernelGGL(k_lookup_level_keys, dim3(nseg, ch.count), dim3(256), 0, st, d_w.as<const int>(), d_ev.as<const uint32_t>(), d_seg.as<const int>(), n,
                           level_bits, ch.count, d_keys.as<uint32_t>());
        const uint32_t key_bits = level_bits + (32u - (uint32_t)__builtin_clz(ch.count));      // the key behind the last lookup's is ch.count << level_bits
        size_t tb = tb_max;
        GL_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tb, d_keys.as<const uint32_t>(), d_keys_out.as<uint32_t>(), d_ev.as<const uint32_t>(),
                                                        d_vals_out.as<uint32_t>(), (int)total, 0, (int)key_bits, st));      // stable: a level keeps the merge order
        hipLaunchKernelGGL(k_lookup_match, dim3((total + 255) / 256), dim3(256), 0, st, d_keys_out.as<const uint32_t>(), d_vals_out.as<const uint32_t>(), total,
                           level_bits, ch.count, n, lk, d_sorted.as<const uint64_t>(), d_cols, d_flag.as<uint32_t>());
        hipLaunchKernelGGL(k_lookup_seg_sums, dim3(nseg, ch.count), dim3(256), 0, st, d_flag.as<const int>(), 2 * n, d_seg.as<int>());
        hipLaunchKernelGGL(k_lookup_seg_scan, dim3(ch.count), dim3(64), 0, st, d_seg.as<int>(), nseg);
        hipLaunchKernelGGL(k_lookup_ranks, dim3(nseg, ch.count), dim3(256), 0, st, d_flag.as<const int>(), d_seg.as<const int>(), 2 * n, d_w.as<int>());
        hipLaunchKernelGGL(k_lookup_left_values, dim3((n + 255) / 256, ch.count), dim3(256), 0, st, d_flag.as<const uint32_t>(), d_w.as<const int>(), lk,
                           d_sorted.as<const uint64_t>(), n, d_canon.as<uint64_t>());
        hipLaunchKernelGGL(k_lookup_left_fill, dim3((n + 255) / 256, ch.count), dim3(256), 0, st, d_flag.as<const uint32_t>(), d_w.as<const int>(), lk,
                           d_canon.as<const uint64_t>(), n, d_cols);
        GL_CHECK_HIP(hipGetLastError());
    }
    return GL_OK;
}

extern "C" int gl_stark_lookup_columns(gl_ctx* c, uint64_t* d_cols, uint32_t num_columns, size_t n_rows, const gl_stark_lookup* lookups, uint32_t count) try {
    GL_REQUIRE(c && d_cols && lookups, GL_ERR_ARG, "gl_stark_lookup_columns: null argument");
    gllookup::Plan plan;
    GL_TRY(gllookup::plan(num_columns, n_rows, lookups, count, &plan));
    GL_TRY(c->activate());
    GlTimed timed(c, "lookup columns");
    DevBuf d_words(c);
    GL_TRY(d_words.alloc(plan.words.size() * 4));
    GL_CHECK_HIP(hipMemcpyAsync(d_words.p, plan.words.data(), plan.words.size() * 4, hipMemcpyHostToDevice, c->stream));
    GL_TRY(gllookup::run(c, d_cols, plan, d_words.as<uint32_t>()));
    GL_CHECK_HIP(gl_stream_wait(c->stream));   // `plan.words` (host source of the async upload) dies here
    return GL_OK;
} catch (...) { return gl_caught(); }
