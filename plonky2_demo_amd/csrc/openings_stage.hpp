// The two halves of gl_verify_openings that the device batch verifier (openings_verify.hip) shares with it (verifier.hip holds the
// definitions; host code, no HIP calls), split the way verify_stage.hpp splits gl_verify: what follows from (gl_fri_params,
// gl_fri_instance without its points) alone -- every size and the place of every leaf, sibling run, cap and coefficient inside the
// decoded word table -- and the per-claim host stage: decode, challenges, proof of work, PrecomputedReducedOpenings.  What is left of a
// claim after that stage, the Merkle paths and the FRI queries of fri/verifier.rs:163-241, reads only the table T, the challenges and
// the claim's caps, on the host (gl_verify_openings) or on the device (k_verify_paths_any, k_verify_openings_queries).
#pragma once
#include "context.hpp"
#include "fri_instance.hpp"
#include <functional>

namespace glopen {

constexpr uint32_t MAX_FRI_ROUNDS = 8, MAX_SLOTS = GL_MAX_FRI_ORACLES + MAX_FRI_ROUNDS;

// One claim's table T: every word of the FriProof in write_fri_proof order, canonical (a hash in a four-word slot: the four elements
// of a HashOut, or the raw 25 bytes of a BytesHash<25>), without the path-length bytes and the proof-of-work witness:
//   commit-phase caps [num_rounds][ncap][4] | per query: per slot its leaf, then its siblings [nsib][4] | final polynomial [final_len][2]
// Slot s < num_oracles: initial tree s; slot num_oracles + r: the step tree of reduction r.  The decode validates every path length,
// so the offsets below hold for every proof that passes it.
struct Shape {
    uint32_t hasher = 0, num_queries = 0, num_rounds = 0, num_oracles = 0, num_batches = 0, cap_height = 0, lgN = 0;
    uint32_t arity_bits[MAX_FRI_ROUNDS] = {};
    size_t ncap = 0, final_len = 0;
    size_t o_fcaps = 0, o_query0 = 0, query_stride = 0, o_final = 0, t_words = 0;
    // offsets relative to the query's first word; slot_leaf_len counts the salt behind the unsalted prefix
    size_t slot_leaf[MAX_SLOTS] = {}, slot_leaf_len[MAX_SLOTS] = {}, slot_sib[MAX_SLOTS] = {}, slot_nsib[MAX_SLOTS] = {};
    // fri_combine_initial's reads: batch b lists the polynomials first[b] .. first[b + 1]; the j-th listed one is the word src[j] of a
    // query's record (slot_leaf[oracle] + polynomial_index: inside the unsalted prefix)
    uint32_t first[GL_MAX_FRI_BATCHES + 1] = {};
    std::vector<uint32_t> src;
    uint32_t num_slots() const { return num_oracles + num_rounds; }
    size_t leaf_at(size_t q, uint32_t slot) const { return o_query0 + q * query_stride + slot_leaf[slot]; }
    size_t sib_at(size_t q, uint32_t slot) const { return o_query0 + q * query_stride + slot_sib[slot]; }
};

// what the queries need of the transcript (fri/challenges.rs:24-64) and of the openings (PrecomputedReducedOpenings, fri/verifier.rs:243-260)
struct Challenges {
    gl2_t alpha, betas[MAX_FRI_ROUNDS], red[GL_MAX_FRI_BATCHES], alpha_len[GL_MAX_FRI_BATCHES], point[GL_MAX_FRI_BATCHES];
    std::vector<uint64_t> x_index;
};

// glfri::check(params, instance, false) with its codes and texts, then the shape
int shape_of(const gl_fri_params* params, const gl_fri_instance* instance, Shape& s);
// gl_verify_openings behind glfri::check up to its query loop, for an instance that passed shape_of: the coset check of `points` (the
// claim's own; the instance's are not read), the argument checks, the decode into T with its rejections, the challenges, the proof of
// work, the reduced openings.  GL_OK: T and ch are filled.  GL_ERR_VERIFY: *check names the rejecting site.
int host_stage(const gl_fri_params& p, const gl_fri_instance& in, const Shape& s, const uint64_t (*points)[2], const uint64_t* caps, const uint64_t* openings,
               gl_challenger* challenger, const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, Challenges& ch, uint32_t* check);

// ---- the device batch verifier's inside (openings_verify.hip), which the STARK batch verifier (stark.hip) drives with
// claims it makes itself ----
// Fills claim i on host lane `lane` (what it points to must live until the same lane's next call).  GL_OK: the claim goes through the
// host stage and, if it passes, to the device.  GL_ERR_VERIFY: judged already, *check says where.  Any other status fails the call.
typedef std::function<int(size_t lane, size_t i, gl_openings_claim& claim, uint32_t* check)> ClaimSource;
int batch_new(gl_ctx* c, const gl_fri_params* params, const gl_fri_instance* instance, uint32_t max_batch, uint32_t host_threads,
              gl_openings_batch_verifier** out);
int batch_verify(gl_openings_batch_verifier* v, size_t count, const ClaimSource& source, int32_t* verdicts, uint32_t* checks);

}  // namespace glopen
