// Batch verification: VerifierCircuitData::verify for many proofs of one circuit (plonk/verifier.rs:15-115).
//
// What runs where.  Per proof the host stage of gl_verify (verify_stage.hpp: decode, transcript, vanishing identity at zeta, proof of
// work, reduced openings) runs on host threads: its sponges are sequential (the public-input hash, the Challenger), so a proof gives a
// device lane nothing to do side by side.  What is left is the query phase of a FRI proof like any other: the circuit's FRI instance
// is the four oracles and two batches of glfri::PlonkInstance (fri_instance.hpp), so the proof's table goes to the batch core of
// openings_verify.hip as it is, with a cap block of constants_sigmas_cap and the proof's three caps.  No kernel lives here.
#include "context.hpp"
#include "verify_stage.hpp"
#include <memory>

struct gl_batch_verifier {
    gl_circuit_desc desc;
    glverify::Shape shape;
    std::vector<uint64_t> cap;                         // as the caller gave it
    uint64_t digest[4];
    std::vector<std::vector<uint64_t>> caps;           // per host lane: the cap, then the proof's three caps
    glopen::BatchCore* core = nullptr;
};

extern "C" void gl_batch_verifier_free(gl_batch_verifier* v) noexcept {
    if (!v) return;
    glopen::core_free(v->core);
    delete v;
}

extern "C" int gl_batch_verifier_new(gl_ctx* c, const gl_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                                     uint32_t max_batch, uint32_t host_threads, gl_batch_verifier** out) try {
    const glopen::Names names = {"gl_batch_verifier", "this description", "batch_verify"};
    GL_REQUIRE(out, GL_ERR_ARG, "gl_batch_verifier_new: null argument");
    *out = nullptr;
    GL_REQUIRE(c && desc && constants_sigmas_cap && circuit_digest, GL_ERR_ARG, "gl_batch_verifier_new: null argument");
    GL_TRY(glopen::check_batch(names, max_batch, host_threads));
    std::unique_ptr<gl_batch_verifier, void (*)(gl_batch_verifier*)> v(new gl_batch_verifier(), gl_batch_verifier_free);      // error paths free everything
    GL_TRY(glverify::shape_of(*desc, SIZE_MAX, v->shape));
    const size_t cap_words = 4 * v->shape.fri.ncap;
    v->desc = *desc;
    v->cap.assign(constants_sigmas_cap, constants_sigmas_cap + cap_words);
    for (int k = 0; k < 4; k++) v->digest[k] = circuit_digest[k];
    v->caps.assign(host_threads ? host_threads : 1, std::vector<uint64_t>(4 * cap_words));
    for (auto& block : v->caps) std::copy(v->cap.begin(), v->cap.end(), block.begin());
    GL_TRY(glopen::core_new(c, v->shape.fri, max_batch, host_threads, names, &v->core));
    *out = v.release();
    return GL_OK;
} catch (...) { return gl_caught(); }

extern "C" int gl_batch_verifier_verify(gl_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count, int32_t* verdicts,
                                        uint32_t* checks) try {
    GL_REQUIRE(v, GL_ERR_ARG, "gl_batch_verifier_verify: null verifier");
    if (!count) return GL_OK;
    GL_REQUIRE(proofs && num_bytes && verdicts, GL_ERR_ARG, "gl_batch_verifier_verify: null argument");
    const gl_circuit_desc& d = v->desc;
    const glverify::Shape& s = v->shape;
    return glopen::core_verify(v->core, count, [&](size_t lane, size_t i, glopen::Lane& L) -> int {
        GL_REQUIRE(proofs[i], GL_ERR_ARG, "gl_batch_verifier_verify: null proof");
        if (!(d.num_query_rounds <= num_bytes[i] / 8 && d.num_public_inputs <= num_bytes[i] / 8)) {      // gl_verify's one check of the description against the proof
            L.verdict = GL_ERR_ARG; L.check = GL_CHECK_DESCRIPTION;
            return GL_OK;
        }
        const int st = glverify::host_stage(d, s, v->cap.data(), v->digest, proofs[i], num_bytes[i], L.T, L.ch, &L.check);
        if (st != GL_OK && st != GL_ERR_VERIFY) return st;
        L.verdict = st;
        if (st == GL_OK) {
            std::vector<uint64_t>& block = v->caps[lane];
            std::copy(L.T.begin() + s.o_caps, L.T.begin() + s.o_caps + 3 * block.size() / 4, block.begin() + block.size() / 4);
            L.caps = block.data();
        }
        return GL_OK;
    }, verdicts, checks);
} catch (...) { return gl_caught(); }
