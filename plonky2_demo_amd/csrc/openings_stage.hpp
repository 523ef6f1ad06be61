// The one FRI verifier (fri/verifier.rs:62-260) as its callers see it (verifier.hip holds the host definitions, openings_verify.hip the
// device core; this header has no HIP calls).  A FRI proof is verified in two halves.  What follows from the description alone is a
// Shape: every size and the place of every leaf, sibling run, cap and coefficient inside the decoded word table.  What a proof adds is
// the table T itself and the Challenges, which a host stage fills: the decode, the challenge draw, the proof of work and
// PrecomputedReducedOpenings.  What is left after the stage, the Merkle paths and the FRI queries of fri/verifier.rs:163-241, reads only
// T, the challenges and the caps, in one query loop on the host (gl_verify, gl_verify_openings) or on the device
// (k_verify_paths_any, k_verify_openings_queries).  There are three stages: glopen::host_stage for any FriInstanceInfo,
// glverify::host_stage (verify_stage.hpp) for a circuit proof, whose instance is the four oracles and two batches of
// glfri::PlonkInstance (fri_instance.hpp), and the STARK stage (stark.hip), which ends in glopen::host_stage.
#pragma once
#include "context.hpp"
#include "fri_instance.hpp"
#include <functional>

namespace glopen {

constexpr uint32_t MAX_FRI_ROUNDS = 8, MAX_SLOTS = GL_MAX_FRI_ORACLES + MAX_FRI_ROUNDS;

// The FriProof's part of a table T: every word in write_fri_proof order, canonical (a hash in a four-word slot: the four elements
// of a HashOut, or the raw 25 bytes of a BytesHash<25>), without the path-length bytes and the proof-of-work witness:
//   commit-phase caps [num_rounds][ncap][4] | per query: per slot its leaf, then its siblings [nsib][4] | final polynomial [final_len][2]
// It starts at o_fcaps: 0 in a claim's table, behind the caps and the openings in a circuit proof's.
// Slot s < num_oracles: initial tree s; slot num_oracles + r: the step tree of reduction r.  The decode validates every path length,
// so the offsets below hold for every proof that passes it.
struct Shape {
    uint32_t hasher = 0, num_queries = 0, num_rounds = 0, num_oracles = 0, num_batches = 0, cap_height = 0, lgN = 0;
    uint32_t arity_bits[MAX_FRI_ROUNDS] = {};
    size_t ncap = 0, final_len = 0;
    size_t o_fcaps = 0, o_query0 = 0, query_stride = 0, o_final = 0;
    size_t t_words = 0;                                // the final polynomial's end; SIZE_MAX: the table does not fit a size_t
    // false when a step tree would be lower than the cap: the decode then rejects every proof (the slots from that tree on stay empty)
    bool paths_fit = true;
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

// The rest of a shape from its counts (hasher .. lgN, arity_bits, ncap, final_len), the words per leaf of every oracle and the
// instance's list of (oracle, polynomial) pairs, batch after batch: the slots, every offset from `base` on, first[] and src[]
void lay_out(Shape& s, const size_t* leaf_lens, const uint32_t* batch_len, const uint32_t* polys, size_t base);

// glfri::check(params, instance, false) with its codes and texts, then the shape
int shape_of(const gl_fri_params* params, const gl_fri_instance* instance, Shape& s);
// gl_verify_openings behind glfri::check up to its query loop, for an instance that passed shape_of: the coset check of `points` (the
// claim's own; the instance's are not read), the argument checks, the decode into T with its rejections, the challenges, the proof of
// work, the reduced openings.  GL_OK: T and ch are filled.  GL_ERR_VERIFY: *check names the rejecting site.
int host_stage(const gl_fri_params& p, const gl_fri_instance& in, const Shape& s, const uint64_t (*points)[2], const uint64_t* caps, const uint64_t* openings,
               gl_challenger* challenger, const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, Challenges& ch, uint32_t* check);

// ---- the device batch core (openings_verify.hip): the query phase of many proofs of one shape ----
// What a host stage leaves on its host lane for proof i: T, ch, the proof's caps [num_oracles][ncap][4] (alive until the same lane's
// next call), and the stage's status and check.  verdict GL_OK: the proof goes to the device.  Anything else is the proof's verdict.
struct Lane {
    std::vector<gl_t> T; Challenges ch; const uint64_t* caps; int32_t verdict; uint32_t check;
    // a host stage's status: GL_OK, GL_ERR_VERIFY and GL_ERR_ARG (the proof's own points or challenger) are verdicts, any other fails the call
    int judged(int st) { verdict = st; return st == GL_OK || st == GL_ERR_VERIFY || st == GL_ERR_ARG ? GL_OK : st; }
};
// the host stage of proof i on lane `lane`; a status other than GL_OK fails the call
typedef std::function<int(size_t lane, size_t i, Lane& L)> Stage;
// how an entry names itself: in the core's refusals ("<entry>_new: ..." about "a proof of <subject>"), and its timing scope
struct Names { const char *entry, *subject, *scope; };
struct BatchCore;
// check_batch: the limits every entry shares (max_batch 1..4096, at most 64 threads); an entry calls it in front of its own checks of
// the description, core_new relies on it.  core_new: arity bits <= 4, a record of at most 2^24 words, a batch of at most 2^31 paths;
// GL_ERR_INTERNAL for a shape whose reads would leave its record
int check_batch(const Names& names, uint32_t max_batch, uint32_t host_threads);
int core_new(gl_ctx* c, const Shape& s, uint32_t max_batch, uint32_t host_threads, const Names& names, BatchCore** out);
void core_free(BatchCore* core) noexcept;
int core_verify(BatchCore* core, size_t count, const Stage& stage, int32_t* verdicts, uint32_t* checks);

// the generic entry's verifier, which the STARK batch verifier (stark.hip) drives with claims it makes itself: glopen::host_stage as
// the core's stage.  `source` fills claim i on host lane `lane` (what it points to must live until the same lane's next call).
// GL_OK: the claim goes through the host stage.  GL_ERR_VERIFY: judged already, *check says where.  Any other status fails the call.
typedef std::function<int(size_t lane, size_t i, gl_openings_claim& claim, uint32_t* check)> ClaimSource;
int batch_new(gl_ctx* c, const gl_fri_params* params, const gl_fri_instance* instance, uint32_t max_batch, uint32_t host_threads,
              gl_openings_batch_verifier** out);
int batch_verify(gl_openings_batch_verifier* v, size_t count, const ClaimSource& source, int32_t* verdicts, uint32_t* checks);

}  // namespace glopen
