// What stark_lookup.hip shares with memory_trace.hip: gl_stark_lookup_columns' body in its two halves, the host plan of a call and
// its launches.  A caller that keeps the plan's words in HBM runs the launches without waiting for the stream.  Host code.
#pragma once
#include "context.hpp"
#include <vector>

namespace gllookup {
struct Chunk {
    uint32_t first, count;                     // lookups [first, first + count) of the call
    uint32_t num_slots, keep;                  // sorted source columns of the chunk; the first `keep` are the previous chunk's
    size_t lk_off, slot_off, seg_off;          // offsets of its tables in the uploaded words
};
struct Plan {
    uint32_t n = 0, lg_n = 0, count = 0, per_chunk = 0, max_slots = 0;
    std::vector<Chunk> chunks;
    std::vector<uint32_t> words;               // every chunk's tables, uploaded once
};
int plan(uint32_t num_columns, size_t n_rows, const gl_stark_lookup* lookups, uint32_t count, Plan* out);
int run(gl_ctx* c, uint64_t* d_cols, const Plan& plan, const uint32_t* d_words);
}  // namespace gllookup
