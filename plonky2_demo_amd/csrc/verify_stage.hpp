// The circuit-proof stage in front of the one FRI verifier (openings_stage.hpp; verifier.hip holds the definitions; host code, no HIP
// calls): what follows from the description alone -- gl_verify's checks of it, the place of the caps, the openings and the public
// inputs inside the decoded word table, and the circuit's FRI instance (glfri::PlonkInstance) as a glopen::Shape over that table -- and
// the per-proof host stage: decode, challenges, the vanishing identity at zeta, the proof of work and the reduced openings.  What is
// left of a proof after that stage is the shared query loop, on the host (gl_verify) or on the device (batch_verify.hip).
#pragma once
#include "openings_stage.hpp"

namespace glverify {

// One proof's table T: every word of the proof in wire order, canonical (a hash in a four-word slot: the four elements of a HashOut, or
// the raw 25 bytes of a BytesHash<25>), without the proof-of-work witness and the public-input count:
//   caps of wires, Z / partial products, quotient [3][ncap][4] | OpeningSet | the FriProof (fri, from fri.o_fcaps on) | public inputs
struct Shape {
    glopen::Shape fri;                                 // oracles: constants_sigmas, wires, Z / partial products / lookups, quotient
    uint32_t lgn = 0;
    size_t num_constants = 0, nlp = 0, num_public_inputs = 0;
    size_t o_caps = 0, o_const = 0, o_sig = 0, o_wires = 0, o_zs = 0, o_zsn = 0, o_lk = 0, o_lkn = 0, o_pp = 0, o_quot = 0, o_pis = 0;
    size_t t_words = 0;                                // SIZE_MAX: the table of this description does not fit a size_t
};

// gl_verify's checks of the description, in its order and with its codes and texts, then the shape.  `num_bytes`: the length of the
// proof the description is held against (two counts must fit it); SIZE_MAX asks for the checks that hold for every proof.
int shape_of(const gl_circuit_desc& d, size_t num_bytes, Shape& s);
// gl_verify up to its query loop.  GL_OK: T and ch are filled (ch.point: zeta, g zeta).  GL_ERR_VERIFY: *check names the rejecting
// site (GL_CHECK_*) and the calling thread's last error holds its text.
int host_stage(const gl_circuit_desc& d, const Shape& s, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
               const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, glopen::Challenges& ch, uint32_t* check);
const char* check_message(uint32_t check) noexcept;

}  // namespace glverify
