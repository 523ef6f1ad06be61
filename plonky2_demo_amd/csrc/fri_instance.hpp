// What gl_fri_combine_instance, gl_prove_openings (prove.hip) and gl_verify_openings (verifier.hip) share: the Challenger's C handle, the
// validation of a FriParams / FriInstanceInfo pair (fri/mod.rs, fri/structure.rs), and the one instance both sides build themselves: a
// circuit's (PlonkInstance, for gl_fri_combine / gl_prove* and gl_verify).  Host code.
#pragma once
#include "context.hpp"
#include "host_circuit.hpp"
#include "proof.hpp"

// C handle of the Challenger for callers of the phase API that have no transcript of their own (C / C++ / Python)
struct gl_challenger { glhost::HostChallenger ch; };

namespace glfri {

enum { MAX_LISTED_POLYS = 65536, SALT_SIZE = 4 };

inline size_t total_polys(const gl_fri_instance& in) { size_t t = 0; for (uint32_t b = 0; b < in.num_batches; b++) t += in.batch_len[b]; return t; }
inline uint32_t salt_of(const gl_fri_params& p, const gl_fri_instance& in, uint32_t o) { return p.hiding && in.oracle_blinding[o] ? SALT_SIZE : 0; }
inline gl2_t point_of(const gl_fri_instance& in, uint32_t b) { return gl2_make(gl_canon(in.points[b][0]), gl_canon(in.points[b][1])); }

// the size of gl_prove_openings' FriProof (write_fri_proof, util/serialization/mod.rs:1568-1582): the params and the instance fix it
inline size_t proof_bytes(const gl_fri_params& p, const gl_fri_instance& in) {
    const size_t hb = hash_wire_bytes(p.hasher), lgN = p.degree_bits + p.rate_bits;
    size_t per_query = 0, lg = lgN, final_len = size_t(1) << p.degree_bits;
    for (uint32_t o = 0; o < in.num_oracles; o++) per_query += 8 * (size_t)(in.oracle_num_polys[o] + salt_of(p, in, o)) + 1 + hb * (lgN - p.cap_height);
    for (unsigned r = 0; r < p.num_fri_rounds; r++) {
        lg -= p.fri_arity_bits[r]; final_len >>= p.fri_arity_bits[r];
        per_query += (size_t(16) << p.fri_arity_bits[r]) + 1 + hb * (lg - p.cap_height);
    }
    return (size_t)p.num_fri_rounds * (hb << p.cap_height) + (size_t)p.num_query_rounds * per_query + 16 * final_len + 8;
}

// a point 7 w with w^N = 1 is an LDE point: the quotient by (X - point) has a pole there (the reference panics dividing by zero)
inline int check_points(const gl_fri_params& p, uint32_t num_batches, const uint64_t (*points)[2]) {
    const gl_t inv7 = gl_inv(GL_MULT_GENERATOR);
    for (uint32_t b = 0; b < num_batches; b++) {
        if (gl_canon(points[b][1]) != 0) continue;
        gl_t w = gl_mul(gl_canon(points[b][0]), inv7);
        for (uint32_t i = 0; i < p.degree_bits + p.rate_bits; i++) w = gl_sqr(w);
        GL_REQUIRE(gl_canon(w) != 1, GL_ERR_ARG, "FRI openings: an opening point lies on the LDE coset");
    }
    return GL_OK;
}

// the checks of include/plonky2_mi355x.h ("Validation"); `prover`: the two calls that fold by 16 only
inline int check(const gl_fri_params* params, const gl_fri_instance* instance, bool prover) {
    GL_REQUIRE(params && instance, GL_ERR_ARG, "FRI openings: null params / instance");
    const gl_fri_params& p = *params; const gl_fri_instance& in = *instance;
    GL_REQUIRE(p.hasher <= GL_HASHER_KECCAK, GL_ERR_ARG, "FRI openings: hasher is 0 (Poseidon) or 1 (Keccak)");
    GL_REQUIRE(p.hiding <= 1, GL_ERR_ARG, "FRI openings: hiding is 0 or 1");
    GL_REQUIRE(p.degree_bits >= 1 && p.rate_bits <= 24 && p.degree_bits <= 24 && p.degree_bits + p.rate_bits <= 24, GL_ERR_ARG,
               "FRI openings: degree_bits >= 1 and an LDE of at most 2^24");
    GL_REQUIRE(p.cap_height <= p.degree_bits + p.rate_bits, GL_ERR_ARG, "FRI openings: cap_height above the LDE's height");
    GL_REQUIRE(p.num_query_rounds >= 1 && p.num_query_rounds <= 256 && p.proof_of_work_bits <= 40 && p.num_fri_rounds <= 8, GL_ERR_ARG,
               "FRI openings: 1..256 query rounds, at most 40 bits of work, at most 8 reductions");
    unsigned total = 0;
    for (unsigned r = 0; r < p.num_fri_rounds; r++) {
        GL_REQUIRE(p.fri_arity_bits[r] >= 1 && p.fri_arity_bits[r] <= 8, GL_ERR_ARG, "FRI openings: arity bits are 1..8");
        total += p.fri_arity_bits[r];
    }
    GL_REQUIRE(total <= p.degree_bits && total + p.cap_height <= p.degree_bits + p.rate_bits, GL_ERR_ARG,
               "FRI total reduction arity is too large");      // circuit_builder.rs:977-980
    GL_REQUIRE(in.num_oracles >= 1 && in.num_oracles <= GL_MAX_FRI_ORACLES, GL_ERR_ARG, "FRI openings: 1..8 oracles");
    GL_REQUIRE(in.num_batches >= 1 && in.num_batches <= GL_MAX_FRI_BATCHES, GL_ERR_ARG, "FRI openings: 1..4 batches");
    for (uint32_t o = 0; o < in.num_oracles; o++)
        GL_REQUIRE(in.oracle_num_polys[o] >= 1 && in.oracle_num_polys[o] <= MAX_LISTED_POLYS && in.oracle_blinding[o] <= 1, GL_ERR_ARG,
                   "FRI openings: an oracle has 1..65536 polynomials, blinding is 0 or 1");
    GL_REQUIRE(in.polys, GL_ERR_ARG, "FRI openings: null polynomial list");
    size_t listed = 0;
    for (uint32_t b = 0; b < in.num_batches; b++) {
        GL_REQUIRE(in.batch_len[b] >= 1 && in.batch_len[b] <= MAX_LISTED_POLYS, GL_ERR_ARG, "FRI openings: an empty batch (or one above 65536 polynomials)");
        listed += in.batch_len[b];
    }
    GL_REQUIRE(listed <= MAX_LISTED_POLYS, GL_ERR_ARG, "FRI openings: more than 65536 listed polynomials");
    for (size_t k = 0; k < listed; k++)
        GL_REQUIRE(in.polys[2 * k] < in.num_oracles && in.polys[2 * k + 1] < in.oracle_num_polys[in.polys[2 * k]], GL_ERR_ARG,
                   "FRI openings: oracle / polynomial index out of range");
    GL_TRY(check_points(p, in.num_batches, in.points));
    if (prover)
        for (unsigned r = 0; r < p.num_fri_rounds; r++) GL_REQUIRE(p.fri_arity_bits[r] == 4, GL_ERR_UNSUPPORTED, "FRI arity must be 16");
    return GL_OK;
}

// A circuit's FriInstanceInfo (fri_all_polys / fri_next_batch_polys, circuit_data.rs:564-597, in FriOpenings order, proof.rs:346-380) without
// its points: oracles constants||sigmas, wires, Z||partial products(||lookups), quotient, the last three blinded (prover.rs:151,218,266);
// batch 0 at zeta = constants and sigmas, wires, the 20 of Z and partial products, the 16 quotient chunks, then the lookup polynomials;
// batch 1 at g zeta = the 2 Zs and the lookup polynomials.  The lookup polynomials come LAST in both batches.  This is the only place
// that spells the order out; it depends on the description alone, a proof writes its two points into a copy of `inst`.
struct PlonkInstance {
    gl_fri_instance inst;
    std::vector<uint32_t> polys;
    PlonkInstance(const PlonkInstance&) = delete;
    explicit PlonkInstance(const gl_circuit_desc& d) : inst() {
        const uint32_t nlk = 2 * d.num_lookup_polys, widths[4] = {d.num_constants + 80, 135, 20 + nlk, 16};
        inst.num_oracles = 4; inst.num_batches = 2;
        for (uint32_t o = 0; o < 4; o++) { inst.oracle_num_polys[o] = widths[o]; inst.oracle_blinding[o] = o != 0; }
        auto add = [&](uint32_t o, uint32_t first, uint32_t count) { for (uint32_t c = first; c < first + count; c++) { polys.push_back(o); polys.push_back(c); } };
        add(0, 0, widths[0]); add(1, 0, 135); add(2, 0, 20); add(3, 0, 16); add(2, 20, nlk);
        inst.batch_len[0] = (uint32_t)(polys.size() / 2);
        add(2, 0, 2); add(2, 20, nlk);
        inst.batch_len[1] = (uint32_t)(polys.size() / 2) - inst.batch_len[0];
        inst.polys = polys.data();
    }
};

}  // namespace glfri
