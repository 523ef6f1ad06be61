// The two halves of gl_verify that the batch verifier (batch_verify.hip) shares with it (verifier.hip holds the definitions; host code,
// no HIP calls): what follows from the description alone -- its checks, every size and the place of every leaf, sibling run, cap and
// coefficient inside the decoded word table -- and the per-proof host stage: decode, challenges, the vanishing identity at zeta and the
// proof of work.  What is left of a proof after that stage, the Merkle paths and the FRI queries of fri/verifier.rs:62-260, reads only
// the table T and the challenge block, on the host (gl_verify) or on the device (k_verify_merkle_paths, k_verify_fri_queries).
#pragma once
#include "context.hpp"

namespace glverify {

constexpr uint32_t MAX_FRI_ROUNDS = 8, NUM_INITIAL_TREES = 4, MAX_SLOTS = NUM_INITIAL_TREES + MAX_FRI_ROUNDS;

// One proof's table T: every word of the proof in wire order, canonical (a hash in a four-word slot: the four elements of a HashOut, or
// the raw 25 bytes of a BytesHash<25>), without the proof-of-work witness and the public-input count.  The decode validates every path
// length, so the offsets below hold for every proof that passes it.
struct Shape {
    uint32_t hasher = 0, num_queries = 0, num_rounds = 0, cap_height = 0, lgn = 0, lgN = 0;
    uint32_t arity_bits[MAX_FRI_ROUNDS] = {};
    size_t ncap = 0, num_constants = 0, nlp = 0, nzp = 0, final_len = 0, num_public_inputs = 0;
    size_t widths[4] = {}, leaf_lens[4] = {};          // polynomials per initial tree / words per leaf (the salt behind them)
    size_t o_caps = 0, o_const = 0, o_sig = 0, o_wires = 0, o_zs = 0, o_zsn = 0, o_lk = 0, o_lkn = 0, o_pp = 0, o_quot = 0, o_fcaps = 0;
    size_t o_query0 = 0, query_stride = 0, o_final = 0, o_pis = 0;
    // slot s < 4: initial tree s; slot 4 + r: the step tree of FRI round r.  Offsets are relative to the query's first word.
    // paths_fit is false when a step tree would be lower than the cap: gl_verify then rejects every proof in the decode
    bool paths_fit = true;
    size_t slot_leaf[MAX_SLOTS] = {}, slot_leaf_len[MAX_SLOTS] = {}, slot_sib[MAX_SLOTS] = {}, slot_nsib[MAX_SLOTS] = {};
    size_t t_words = 0;                                // SIZE_MAX: the table of this description does not fit a size_t
    uint32_t num_slots() const { return NUM_INITIAL_TREES + num_rounds; }
    size_t leaf_at(size_t q, uint32_t slot) const { return o_query0 + q * query_stride + slot_leaf[slot]; }
    size_t sib_at(size_t q, uint32_t slot) const { return o_query0 + q * query_stride + slot_sib[slot]; }
};

// what the queries need of the transcript (fri/challenges.rs:24-64) and of the openings (PrecomputedReducedOpenings, fri/verifier.rs:243-260)
struct Challenges {
    gl2_t zeta, gzeta, fri_alpha, fri_betas[MAX_FRI_ROUNDS], red0, red1, alpha_shift;
    std::vector<uint64_t> x_index;
};
constexpr size_t CHALLENGE_WORDS = 2 * (6 + MAX_FRI_ROUNDS);      // the block above as words, in front of the x_index

// gl_verify's checks of the description, in its order and with its codes and texts, then the shape.  `num_bytes`: the length of the
// proof the description is held against (two counts must fit it); SIZE_MAX asks for the checks that hold for every proof.
int shape_of(const gl_circuit_desc& d, size_t num_bytes, Shape& s);
// gl_verify up to the proof of work.  GL_OK: T and ch are filled.  GL_ERR_VERIFY: *check names the rejecting site (GL_CHECK_*) and
// the calling thread's last error holds its text.
int host_stage(const gl_circuit_desc& d, const Shape& s, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
               const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, Challenges& ch, uint32_t* check);
const char* check_message(uint32_t check) noexcept;

}  // namespace glverify
