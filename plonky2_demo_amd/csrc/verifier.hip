// Native verifier for proofs of circuits over the demo's gate set (host code, as in the reference:
// plonky2/src/plonk/verifier.rs:15-115, plonk/get_challenges.rs:26-87, plonk/vanishing_poly.rs:54-160,
// plonk/validate_shape.rs, fri/verifier.rs:21-260, fri/validate_shape.rs, hash/merkle_proofs.rs:54-75).
//
// Input is exactly what the reference's `VerifierCircuitData::verify` sees: CommonCircuitData (here the gl_circuit_desc),
// VerifierOnlyCircuitData (constants_sigmas_cap, circuit_digest) and ProofWithPublicInputs::to_bytes().  The proof is
// checked in place: one pass turns the byte string into a flat table of canonical words plus offsets, and every later
// step indexes that table.  No GPU is involved.  The checks of the description and the per-proof stage up to the queries are functions
// of their own (verify_stage.hpp): the batch verifier (batch_verify.hip) runs the same ones and gives the queries to the device.  The
// FRI half -- decode, challenge draw, reduced openings, query loop -- is one set of functions for a circuit proof (whose instance is
// glfri::PlonkInstance, fri_instance.hpp, the prover's too) and for a FriProof of any FriInstanceInfo (gl_verify_openings at the end of
// this file; openings_stage.hpp).
#include "context.hpp"
#include "host_circuit.hpp"
#include "fri_instance.hpp"
#include "openings_stage.hpp"
#include "verify_stage.hpp"

namespace {

typedef gl2_t E;                                      // F_p[X]/(X^2 - 7)
inline E e_of(gl_t a) { return gl2_make(a, 0); }
inline E e_add(E x, E y) { return gl2_add(x, y); }
inline E e_sub(E x, E y) { return gl2_sub(x, y); }
inline E e_mul(E x, E y) { return gl2_mul(x, y); }
inline E e_scale(E x, gl_t s) { return gl2_scalar(x, s); }
inline bool e_eq(E x, E y) { x = gl2_canon(x); y = gl2_canon(y); return x.a == y.a && x.b == y.b; }
inline E e_sbox(E x) { E x2 = e_mul(x, x), x4 = e_mul(x2, x2); return e_mul(e_mul(x, x2), x4); }
inline E e_pow2k(E x, unsigned k) { for (unsigned i = 0; i < k; i++) x = e_mul(x, x); return x; }
inline E e_pow(E x, size_t k) { E r = e_of(1); for (; k; k >>= 1, x = e_mul(x, x)) if (k & 1) r = e_mul(r, x); return r; }

// ---- Merkle path to a cap (hash/merkle_proofs.rs:54-75; leaf hash plonk/config.rs:55-66) ----
// `hasher`: C::Hasher.  A HashOut's words compare as field elements; a BytesHash<25>'s as the bytes they are.
bool path_opens_to_cap(uint32_t hasher, const gl_t* leaf, size_t leaf_len, size_t index, const gl_t* siblings, size_t nsib, const gl_t* cap, size_t cap_len) {
    gl_t cur[4];
    glhost::hash_or_noop(hasher, leaf, leaf_len, cur);
    for (size_t l = 0; l < nsib; l++) {
        const gl_t* sib = siblings + 4 * l;
        gl_t out[4];
        if (index & 1) glhost::two_to_one(hasher, sib, cur, out); else glhost::two_to_one(hasher, cur, sib, out);
        for (int k = 0; k < 4; k++) cur[k] = out[k];
        index >>= 1;
    }
    if (index >= cap_len) return false;
    for (int k = 0; k < 4; k++) if (cur[k] != (hasher == GL_HASHER_KECCAK ? cap[4 * index + k] : gl_canon(cap[4 * index + k]))) return false;
    return true;
}

// compute_evaluation (fri/verifier.rs:21-47): the degree < arity interpolant through the coset of `subgroup_x`, at beta; `evals`: the
// step's 2^ab extension values (a, b) in bit-reversed order, `within` = x_index_within_coset
gl2_t compute_evaluation(gl_t subgroup_x, size_t within, unsigned ab, const gl_t* evals, gl2_t beta) {
    const size_t arity = size_t(1) << ab;
    const gl_t g = glhost::root_of_unity(ab);
    size_t wrev = 0;
    for (unsigned i = 0; i < ab; i++) wrev |= ((within >> i) & 1) << (ab - 1 - i);
    const gl_t start = gl_canon(gl_mul(subgroup_x, gl_exp(g, arity - wrev)));      // coset_start = x * g^{-rev(within)}
    std::vector<gl_t> pts(arity);
    { gl_t y = 1; for (size_t k = 0; k < arity; k++) { pts[k] = gl_canon(gl_mul(start, y)); y = gl_mul(y, g); } }
    E acc = e_of(0);
    for (size_t a = 0; a < arity; a++) {
        size_t arev = 0;
        for (unsigned i = 0; i < ab; i++) arev |= ((a >> i) & 1) << (ab - 1 - i);      // evals are stored in bit-reversed order
        E numer = e_of(1); gl_t denom = 1;
        for (size_t b = 0; b < arity; b++) if (b != a) { numer = e_mul(numer, e_sub(beta, e_of(pts[b]))); denom = gl_mul(denom, gl_sub(pts[a], pts[b])); }
        acc = e_add(acc, e_mul(gl2_make(evals[2 * arev], evals[2 * arev + 1]), e_scale(numer, gl_inv(denom))));
    }
    return acc;
}

// ---- the demo's gates over the extension field ----
// Poseidon layers on extension elements: every layer is F_p-linear except the S-box (hash/poseidon.rs:200-214,264-274,
// 311-366,429-450).  The partial rounds use this build's derived sparse factorisation; the constraint polynomials do not
// depend on the factorisation (only lane 0 meets the S-box, and lane 0 is the same in every factorisation).
void ext_mds(E (&s)[12]) {
    static const uint32_t circ[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};
    E out[12];
    for (int r = 0; r < 12; r++) {
        E acc = e_of(0);
        for (int i = 0; i < 12; i++) acc = e_add(acc, e_scale(s[(i + r) % 12], circ[i]));
        if (r == 0) acc = e_add(acc, e_scale(s[0], 8));
        out[r] = acc;
    }
    for (int i = 0; i < 12; i++) s[i] = out[i];
}
void ext_add_round_constants(E (&s)[12], int round) { for (int i = 0; i < 12; i++) s[i] = e_add(s[i], e_of(POSEIDON_RC[12 * round + i])); }

// the POSEIDON_GATE_CONSTRAINTS constraints of gates/poseidon.rs:113-191 on the row `w` (135 extension values); returns them in order
void poseidon_gate_constraints(const E* w, E* out) {
    using namespace glhost;
    int c = 0;
    const E swap = w[PW_SWAP];
    out[c++] = e_mul(swap, e_sub(swap, e_of(1)));
    for (int i = 0; i < 4; i++) out[c++] = e_sub(e_mul(swap, e_sub(w[PW_INPUT + 4 + i], w[PW_INPUT + i])), w[PW_DELTA + i]);
    E s[12];
    for (int i = 0; i < 4; i++) { s[i] = e_add(w[PW_INPUT + i], w[PW_DELTA + i]); s[4 + i] = e_sub(w[PW_INPUT + 4 + i], w[PW_DELTA + i]); s[8 + i] = w[PW_INPUT + 8 + i]; }
    int round = 0;
    for (int r = 0; r < 4; r++, round++) {
        ext_add_round_constants(s, round);
        if (r) for (int i = 0; i < 12; i++) { const E in = w[PW_FULL0 + 12 * (r - 1) + i]; out[c++] = e_sub(s[i], in); s[i] = in; }
        for (int i = 0; i < 12; i++) s[i] = e_sbox(s[i]);
        ext_mds(s);
    }
    for (int i = 0; i < 12; i++) s[i] = e_add(s[i], e_of(POSEIDON_PARTIAL_FIRST_RC[i]));
    {
        E t[12]; t[0] = s[0];
        for (int col = 1; col < 12; col++) {
            E acc = e_of(0);
            for (int r = 1; r < 12; r++) acc = e_add(acc, e_scale(s[r], POSEIDON_PARTIAL_INIT[(r - 1) * 11 + (col - 1)]));
            t[col] = acc;
        }
        for (int i = 0; i < 12; i++) s[i] = t[i];
    }
    for (int r = 0; r < POSEIDON_PARTIAL_ROUNDS; r++) {
        const E in = w[PW_PARTIAL + r];
        out[c++] = e_sub(s[0], in);
        const E s0 = e_add(e_sbox(in), e_of(POSEIDON_PARTIAL_RC[r]));
        E d = e_scale(s0, 25);
        for (int i = 1; i < 12; i++) d = e_add(d, e_scale(s[i], POSEIDON_PARTIAL_ROW[r * 11 + i - 1]));
        for (int i = 1; i < 12; i++) s[i] = e_add(s[i], e_scale(s0, POSEIDON_PARTIAL_COL[r * 11 + i - 1]));
        s[0] = d;
    }
    round += POSEIDON_PARTIAL_ROUNDS;
    for (int r = 0; r < 4; r++, round++) {
        ext_add_round_constants(s, round);
        for (int i = 0; i < 12; i++) { const E in = w[PW_FULL1 + 12 * r + i]; out[c++] = e_sub(s[i], in); s[i] = in; }
        for (int i = 0; i < 12; i++) s[i] = e_sbox(s[i]);
        ext_mds(s);
    }
    for (int i = 0; i < 12; i++) out[c++] = e_sub(s[i], w[PW_OUTPUT + i]);
}

// ExtensionAlgebra<F_p^2, 2> (field/src/extension/algebra.rs:11-26,113-131): a + b X with X^2 = W = 7, the components themselves in F_p^2
struct Alg { E a, b; };
inline Alg alg_mul(const Alg& x, const Alg& y) {
    return Alg{e_add(e_mul(x.a, y.a), e_scale(e_mul(x.b, y.b), glhost::MULT_GEN /* W = 7 */)), e_add(e_mul(x.a, y.b), e_mul(x.b, y.a))};
}

// The constraints of one gate of `type` (`param`: gl_circuit_desc.gate_params) on the row `wires` (135 extension values), in order, into
// tmp[GL_MAX_GATE_CONSTRAINTS]; returns their number, which gl_verify holds against gate_num_constraints.  An unknown type has none
// (gl_verify refuses it beforehand).
size_t gate_constraints_at(uint8_t type, uint8_t param, const E* wires, const E* gate_consts, const gl_t* pi_hash, E* tmp) {
    size_t cnt = 0;
    switch (type) {
        case glhost::G_NOOP: case glhost::G_LOOKUP: case glhost::G_LOOKUP_TABLE: break;          // no main-trace constraints (lookup.rs:72-75)
        case glhost::G_CONSTANT: cnt = 2; for (int i = 0; i < 2; i++) tmp[i] = e_sub(gate_consts[i], wires[i]); break;                        // constant.rs:59-66
        case glhost::G_PUBLIC_INPUT: cnt = 4; for (int i = 0; i < 4; i++) tmp[i] = e_sub(wires[i], e_of(pi_hash[i])); break;                     // public_input.rs:44-49
        case glhost::G_ARITHMETIC: cnt = 20;                                                                                                    // arithmetic_base.rs:72-92
            for (int i = 0; i < 20; i++) tmp[i] = e_sub(wires[4 * i + 3], e_add(e_mul(e_mul(wires[4 * i], wires[4 * i + 1]), gate_consts[0]), e_mul(wires[4 * i + 2], gate_consts[1])));
            break;
        case glhost::G_BASE_SUM: {                                                                                                              // base_sum.rs:63-76, B = 2
            cnt = 1 + glhost::BASE_SUM_LIMBS;
            E computed = e_of(0);                                                                                                                // reduce_with_powers(limbs, 2)
            for (int i = glhost::BASE_SUM_LIMBS; i-- > 0;) computed = e_add(e_add(computed, computed), wires[1 + i]);
            tmp[0] = e_sub(computed, wires[0]);
            for (int i = 0; i < glhost::BASE_SUM_LIMBS; i++) tmp[1 + i] = e_mul(wires[1 + i], e_sub(wires[1 + i], e_of(1)));
            break;
        }
        case glhost::G_RANDOM_ACCESS: {                                                                                                         // random_access.rs:139-184
            const glhost::RandomAccessLayout ra(param);
            for (uint32_t copy = 0; copy < ra.num_copies; copy++) {
                std::vector<E> items(ra.vec_size);
                for (uint32_t i = 0; i < ra.vec_size; i++) items[i] = wires[ra.wire_list_item(i, copy)];
                for (uint32_t i = 0; i < ra.bits; i++) { const E b = wires[ra.wire_bit(i, copy)]; tmp[cnt++] = e_mul(b, e_sub(b, e_of(1))); }
                E rec = e_of(0);
                for (uint32_t i = ra.bits; i-- > 0;) rec = e_add(e_add(rec, rec), wires[ra.wire_bit(i, copy)]);
                tmp[cnt++] = e_sub(rec, wires[ra.wire_access_index(copy)]);
                for (uint32_t i = 0; i < ra.bits; i++) {                                                                                         // fold the list by bit i
                    const E b = wires[ra.wire_bit(i, copy)];
                    for (size_t j = 0; 2 * j + 1 < items.size(); j++) items[j] = e_add(items[2 * j], e_mul(b, e_sub(items[2 * j + 1], items[2 * j])));
                    items.resize(items.size() / 2);
                }
                tmp[cnt++] = e_sub(items[0], wires[ra.wire_claimed_element(copy)]);
            }
            for (uint32_t i = 0; i < ra.num_extra_constants; i++) tmp[cnt++] = e_sub(gate_consts[i], wires[ra.wire_extra_constant(i)]);
            break;
        }
        case glhost::G_EXPONENTIATION: {                                                                                                        // exponentiation.rs:88-124
            const int n = glhost::EXP_POWER_BITS;
            cnt = n + 1;
            for (int i = 0; i < n; i++) {                                                                                                        // square-and-multiply, bits big-endian
                const E prev = i == 0 ? e_of(1) : e_mul(wires[2 + n + i - 1], wires[2 + n + i - 1]);
                const E bit = wires[1 + (n - 1 - i)];
                tmp[i] = e_sub(e_mul(prev, e_add(e_mul(bit, wires[0]), e_sub(e_of(1), bit))), wires[2 + n + i]);
            }
            tmp[n] = e_sub(wires[1 + n], wires[2 + n + n - 1]);
            break;
        }
        // The extension-field gates: at zeta every wire is itself in F_p^2, so a wire pair is an element (A0, A1) of the ExtensionAlgebra
        // F_p^2[X]/(X^2 - 7) (field/src/extension/algebra.rs:113-131: W = 7 embedded), and a constraint's two components enter the sum
        // in order (to_basefield_array).
        case glhost::G_ARITHMETIC_EXT: {                                                                                                        // arithmetic_extension.rs:68-90
            for (int i = 0; i < glhost::ARITH_EXT_OPS; i++) {
                const E* w = wires + 8 * i;                                                                                               // m0, m1, addend, output
                const Alg prod = alg_mul(Alg{w[0], w[1]}, Alg{w[2], w[3]});
                tmp[cnt++] = e_sub(w[6], e_add(e_mul(prod.a, gate_consts[0]), e_mul(w[4], gate_consts[1])));
                tmp[cnt++] = e_sub(w[7], e_add(e_mul(prod.b, gate_consts[0]), e_mul(w[5], gate_consts[1])));
            }
            break;
        }
        case glhost::G_MUL_EXT: {                                                                                                               // multiplication_extension.rs:65-84
            for (int i = 0; i < glhost::MUL_EXT_OPS; i++) {
                const E* w = wires + 6 * i;                                                                                               // m0, m1, output
                const Alg prod = alg_mul(Alg{w[0], w[1]}, Alg{w[2], w[3]});
                tmp[cnt++] = e_sub(w[4], e_mul(prod.a, gate_consts[0]));
                tmp[cnt++] = e_sub(w[5], e_mul(prod.b, gate_consts[0]));
            }
            break;
        }
        case glhost::G_REDUCING: case glhost::G_REDUCING_EXT: {                                                          // reducing.rs:77-103, reducing_extension.rs:80-104
            // wires 0-1 output, 2-3 alpha, 4-5 old_acc, the coefficients (one wire each / two wires each), the accumulators; the last
            // accumulator is the output
            const bool ext = type == glhost::G_REDUCING_EXT;
            const int nc = ext ? glhost::REDUCING_EXT_COEFFS : glhost::REDUCING_COEFFS, acc0 = 6 + (ext ? 2 : 1) * nc;
            const Alg alpha{wires[2], wires[3]};
            Alg acc{wires[4], wires[5]};
            for (int i = 0; i < nc; i++) {
                const int aw = i == nc - 1 ? 0 : acc0 + 2 * i;
                const Alg acc_i{wires[aw], wires[aw + 1]};
                const Alg coeff = ext ? Alg{wires[6 + 2 * i], wires[7 + 2 * i]} : Alg{wires[6 + i], e_of(0)};
                const Alg t = alg_mul(acc, alpha);
                tmp[cnt++] = e_sub(e_add(t.a, coeff.a), acc_i.a);
                tmp[cnt++] = e_sub(e_add(t.b, coeff.b), acc_i.b);
                acc = acc_i;
            }
            break;
        }
        case glhost::G_POSEIDON: cnt = glhost::POSEIDON_GATE_CONSTRAINTS; poseidon_gate_constraints(wires, tmp); break;
    }
    return cnt;
}

struct Cursor {                                        // little-endian reader over the proof bytes
    const uint8_t* p; size_t len, pos = 0; bool ok = true;
    Cursor(const uint8_t* b, size_t n) : p(b), len(n) {}
    uint64_t u64() {
        if (pos + 8 > len) { ok = false; return 0; }
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= (uint64_t)p[pos + i] << (8 * i);
        pos += 8;
        return v;
    }
    unsigned u8() { if (pos >= len) { ok = false; return 0; } return p[pos++]; }
};

// The decode: proof bytes into the table T, all words in wire order.  Like the reference's read_field (from_canonical_u64 without a
// range check in release builds) a word >= p is taken mod p.  Both readers return where their words start; once the bytes have run
// out (in.ok false) nothing more is read, and what T holds from there on is not looked at: the caller rejects the proof as truncated.
struct Reader {
    Cursor in; uint32_t hasher; std::vector<gl_t>& T;
    Reader(const uint8_t* b, size_t n, uint32_t h, std::vector<gl_t>& table) : in(b, n), hasher(h), T(table) { T.clear(); T.reserve(n / 8 + 8); }
    size_t words(size_t k) {                           // one bounds check and one resize for the run: the decode is a proof's every word
        const size_t at = T.size();
        if (!in.ok) return at;
        if (k > (in.len - in.pos) / 8) { in.ok = false; return at; }
        T.resize(at + k);
        Cursor run(in.p + in.pos, 8 * k);
        for (gl_t* w = T.data() + at; run.pos < run.len; w++) *w = gl_canon(run.u64());
        in.pos += 8 * k;
        return at;
    }
    // read_hash (util/serialization/mod.rs:1332-1338): k hashes into four-word slots -- a HashOut's four elements, or the 25 bytes of a
    // BytesHash<25> (raw words, zero padding)
    size_t hashes(size_t k) {
        if (hasher != GL_HASHER_KECCAK) return words(4 * k);
        size_t at = T.size();
        for (size_t i = 0; i < k && in.ok; i++) { for (int w = 0; w < 3; w++) T.push_back(in.u64()); T.push_back(in.u8()); }
        return at;
    }
};

// every rejection goes through here: the code names the site, the table below holds its text
int reject(uint32_t check, uint32_t* out = nullptr) {
    if (out) *out = check;
    return gl_fail(GL_ERR_VERIFY, glverify::check_message(check), __FILE__, __LINE__);
}

// a + b and a * b of sizes, SIZE_MAX once anything overflowed (a caller-filled description may hold any count)
inline size_t sat_add(size_t a, size_t b) { size_t r; return a == SIZE_MAX || b == SIZE_MAX || __builtin_add_overflow(a, b, &r) ? SIZE_MAX : r; }
inline size_t sat_mul(size_t a, size_t b) { size_t r; return a == SIZE_MAX || b == SIZE_MAX || __builtin_mul_overflow(a, b, &r) ? SIZE_MAX : r; }

// ---- verify_fri_proof (fri/verifier.rs:62-241, fri/challenges.rs:24-64, fri/validate_shape.rs) on a table T, for the host stages
// of a circuit proof and of a generic claim and for the two entries' query loop ----
// The FriProof in write_fri_proof order (util/serialization/mod.rs:1568-1582) up to its final polynomial, appended to T; the check of
// a path of the wrong length, or GL_CHECK_ACCEPTED (the caller then looks at rd.in.ok)
uint32_t decode_fri_proof(Reader& rd, const glopen::Shape& s) {
    (void)rd.hashes((size_t)s.num_rounds * s.ncap);
    for (uint32_t q = 0; q < s.num_queries && rd.in.ok; q++) {
        unsigned init_nsib[GL_MAX_FRI_ORACLES];
        for (uint32_t o = 0; o < s.num_oracles; o++) {
            (void)rd.words(s.slot_leaf_len[o]);
            init_nsib[o] = rd.in.u8(); (void)rd.hashes(init_nsib[o]);
        }
        unsigned lg_cur = s.lgN;
        for (unsigned r = 0; r < s.num_rounds; r++) {
            (void)rd.words(size_t(2) << s.arity_bits[r]);
            const unsigned nsib = rd.in.u8(); (void)rd.hashes(nsib);
            lg_cur -= s.arity_bits[r];
            if (rd.in.ok && nsib + s.cap_height != lg_cur) return GL_CHECK_STEP_PATH_LENGTH;
        }
        for (uint32_t o = 0; o < s.num_oracles && rd.in.ok; o++)
            if (init_nsib[o] + s.cap_height != s.lgN) return GL_CHECK_INITIAL_PATH_LENGTH;
    }
    (void)rd.words(2 * s.final_len);
    return GL_CHECK_ACCEPTED;
}

// FriChallenges (fri/challenges.rs:24-64) from the transcript behind the observed openings: alpha, per reduction its cap and beta,
// the final polynomial, the proof-of-work witness, the query indices.  Returns the proof-of-work response for pow_holds.
gl_t draw_fri_challenges(glhost::HostChallenger& tr, const glopen::Shape& s, const gl_t* T, gl_t pow_witness, glopen::Challenges& ch) {
    ch.alpha = tr.challenge_ext();
    for (unsigned r = 0; r < s.num_rounds; r++) { tr.observe_hashes(s.hasher, T + s.o_fcaps + (size_t)r * 4 * s.ncap, s.ncap); ch.betas[r] = tr.challenge_ext(); }
    for (unsigned r = s.num_rounds; r < glopen::MAX_FRI_ROUNDS; r++) ch.betas[r] = e_of(0);
    tr.observe_many(T + s.o_final, 2 * s.final_len);
    tr.observe(pow_witness);
    const gl_t pow_response = tr.challenge();
    ch.x_index.resize(s.num_queries);
    for (auto& x : ch.x_index) x = tr.challenge() % (uint64_t(1) << s.lgN);
    return pow_response;
}
inline bool pow_holds(gl_t pow_response, uint32_t bits) { return pow_response == 0 || (unsigned)__builtin_clzll(pow_response) >= bits; }

// PrecomputedReducedOpenings (fri/verifier.rs:243-260): per batch Horner in alpha over its opened values (`openings`: extension
// values as word pairs, flat in batch order); alpha^len of each batch; its point
void reduce_openings(const glopen::Shape& s, const uint64_t* openings, const uint64_t (*points)[2], glopen::Challenges& ch) {
    for (uint32_t b = 0; b < GL_MAX_FRI_BATCHES; b++) {
        E acc = e_of(0);
        if (b < s.num_batches)
            for (size_t j = s.first[b + 1]; j-- > s.first[b];) acc = e_add(e_mul(acc, ch.alpha), gl2_make(gl_canon(openings[2 * j]), gl_canon(openings[2 * j + 1])));
        ch.red[b] = acc; ch.alpha_len[b] = b < s.num_batches ? e_pow(ch.alpha, s.first[b + 1] - s.first[b]) : e_of(1);
        ch.point[b] = b < s.num_batches ? gl2_make(gl_canon(points[b][0]), gl_canon(points[b][1])) : e_of(0);
    }
}

// The queries (fri/verifier.rs:163-241) of a proof that passed a host stage; k_verify_paths_any and k_verify_openings_queries are this
// loop on the device.  caps[o]: the cap of initial tree o.
int verify_fri_queries(const glopen::Shape& s, const gl_t* T, const glopen::Challenges& ch, const gl_t* const caps[], uint32_t* check) {
    auto ext_at = [&](size_t off, size_t i) { return gl2_make(T[off + 2 * i], T[off + 2 * i + 1]); };
    const gl_t wN = glhost::root_of_unity(s.lgN);
    const E alpha = ch.alpha;
    const uint32_t* src = s.src.data();
    for (uint32_t q = 0; q < s.num_queries; q++) {
        size_t x = ch.x_index[q];
        for (uint32_t o = 0; o < s.num_oracles; o++)
            if (!path_opens_to_cap(s.hasher, &T[s.leaf_at(q, o)], s.slot_leaf_len[o], x, &T[s.sib_at(q, o)], s.slot_nsib[o], caps[o], s.ncap))
                return reject(GL_CHECK_INITIAL_MERKLE, check);
        // subgroup_x = g * w_N^{reverse_bits(x_index)} (fri/verifier.rs:183-186)
        size_t rev = 0;
        for (unsigned i = 0; i < s.lgN; i++) rev |= ((x >> i) & 1) << (s.lgN - 1 - i);
        gl_t subgroup_x = gl_canon(gl_mul(GL_MULT_GENERATOR, gl_exp(wN, rev)));
        // fri_combine_initial (fri/verifier.rs:122-161): per batch Horner in alpha from its last polynomial to its first.  A polynomial's
        // index is below its oracle's column count, so only the unsalted prefix of a leaf is read (unsalted_eval)
        const gl_t* Q = &T[s.o_query0 + q * s.query_stride];
        const E sx = e_of(subgroup_x);
        E eval = e_of(0);
        for (uint32_t b = 0; b < s.num_batches; b++) {
            E h = e_of(0);
            for (size_t j = s.first[b + 1], j0 = s.first[b]; j-- > j0;) h = e_add(e_mul(h, alpha), e_of(Q[src[j]]));
            eval = e_add(e_mul(eval, ch.alpha_len[b]), e_mul(e_sub(h, ch.red[b]), gl2_inv(e_sub(sx, ch.point[b]))));
        }
        for (unsigned r = 0; r < s.num_rounds; r++) {
            const unsigned ab = s.arity_bits[r];
            const uint32_t slot = s.num_oracles + r;
            const size_t arity = size_t(1) << ab, coset = x >> ab, within = x & (arity - 1), leaf = s.leaf_at(q, slot);
            if (!e_eq(ext_at(leaf, within), eval)) return reject(GL_CHECK_FRI_CONSISTENCY, check);
            eval = compute_evaluation(subgroup_x, within, ab, &T[leaf], ch.betas[r]);
            if (!path_opens_to_cap(s.hasher, &T[leaf], s.slot_leaf_len[slot], coset, &T[s.sib_at(q, slot)], s.slot_nsib[slot], &T[s.o_fcaps + (size_t)r * 4 * s.ncap], s.ncap))
                return reject(GL_CHECK_STEP_MERKLE, check);
            for (unsigned i = 0; i < ab; i++) subgroup_x = gl_sqr(subgroup_x);
            x = coset;
        }
        E fin = e_of(0);
        const E sxf = e_of(gl_canon(subgroup_x));
        for (size_t i = s.final_len; i-- > 0;) fin = e_add(e_mul(fin, sxf), ext_at(s.o_final, i));
        if (!e_eq(fin, eval)) return reject(GL_CHECK_FINAL_POLY, check);
    }
    return GL_OK;
}

}  // namespace

void glopen::lay_out(Shape& s, const size_t* leaf_lens, const uint32_t* batch_len, const uint32_t* polys, size_t base) {
    size_t in_query = 0;
    unsigned lg_cur = s.lgN;
    for (uint32_t slot = 0; slot < s.num_slots(); slot++) {
        if (slot >= s.num_oracles) {
            lg_cur -= s.arity_bits[slot - s.num_oracles];
            if (lg_cur < s.cap_height) { s.paths_fit = false; break; }
        }
        s.slot_leaf[slot] = in_query; s.slot_leaf_len[slot] = slot < s.num_oracles ? leaf_lens[slot] : size_t(2) << s.arity_bits[slot - s.num_oracles];
        s.slot_nsib[slot] = lg_cur - s.cap_height;
        s.slot_sib[slot] = sat_add(in_query, s.slot_leaf_len[slot]);
        in_query = sat_add(s.slot_sib[slot], 4 * s.slot_nsib[slot]);
    }
    s.query_stride = in_query;
    s.o_fcaps = base;
    s.o_query0 = sat_add(base, (size_t)s.num_rounds * 4 * s.ncap);
    s.o_final = sat_add(s.o_query0, sat_mul(in_query, s.num_queries));
    s.t_words = sat_add(s.o_final, 2 * s.final_len);
    for (uint32_t b = 0; b < s.num_batches; b++) s.first[b + 1] = s.first[b] + batch_len[b];
    s.src.resize(s.first[s.num_batches]);
    for (size_t j = 0; j < s.src.size(); j++) s.src[j] = (uint32_t)(s.slot_leaf[polys[2 * j]] + polys[2 * j + 1]);
}

const char* glverify::check_message(uint32_t check) noexcept {
    switch (check) {
        case GL_CHECK_ACCEPTED: return "";
        case GL_CHECK_VERIFIER_DATA: return "malformed verifier data: a 25-byte hash with non-zero padding bytes";
        case GL_CHECK_STEP_PATH_LENGTH: return "malformed proof: FRI step Merkle path has the wrong length";
        case GL_CHECK_INITIAL_PATH_LENGTH: return "malformed proof: initial Merkle path has the wrong length";
        case GL_CHECK_TRUNCATED: return "malformed proof: truncated";
        case GL_CHECK_PUBLIC_INPUT_COUNT: return "malformed proof: wrong number of public inputs";
        case GL_CHECK_LENGTH: return "malformed proof: length mismatch";
        case GL_CHECK_VANISHING: return "vanishing polynomial identity fails at zeta";
        case GL_CHECK_POW: return "invalid proof of work witness";
        case GL_CHECK_INITIAL_MERKLE: return "initial Merkle proof fails";
        case GL_CHECK_FRI_CONSISTENCY: return "FRI consistency check fails";
        case GL_CHECK_STEP_MERKLE: return "FRI step Merkle proof fails";
        case GL_CHECK_FINAL_POLY: return "final polynomial evaluation is invalid";
        case GL_CHECK_DESCRIPTION: return "gl_verify: a count of the description exceeds what the proof bytes can hold";
        case GL_CHECK_CTL: return "cross-table lookup verification failed: the looking tables' Z products differ from the looked table's";
    }
    return "unknown check";
}

int glverify::shape_of(const gl_circuit_desc& d, size_t num_bytes, Shape& s) {
    GL_REQUIRE(d.num_wires == 135 && d.num_routed_wires == 80 && d.num_challenges == 2 && d.quotient_degree_factor == 8 && d.rate_bits == 3,
               GL_ERR_UNSUPPORTED, "gl_verify: only standard_recursion_config circuits are supported");
    GL_REQUIRE(d.num_gates >= 1 && d.num_gates <= GL_MAX_GATES, GL_ERR_ARG, "gl_verify: bad gate count");
    { const char* why = glhost::lookup_shape_error(d); GL_REQUIRE(!why, GL_ERR_UNSUPPORTED, why); }
    GL_REQUIRE(d.zero_knowledge <= 1 && (!d.zero_knowledge || !d.num_luts), GL_ERR_UNSUPPORTED, "gl_verify: zero knowledge is 0 / 1 and not together with lookups");
    GL_REQUIRE(d.hasher <= GL_HASHER_KECCAK, GL_ERR_ARG, "gl_verify: hasher is 0 (Poseidon) or 1 (Keccak)");
    GL_REQUIRE(d.num_selectors >= 1 && d.num_constants == d.num_selectors + d.num_lookup_selectors + 2 && d.num_fri_rounds <= 8 &&
               d.degree_bits >= 1 && d.degree_bits + d.rate_bits <= 32 && d.cap_height <= d.degree_bits + d.rate_bits && d.num_query_rounds >= 1,
               GL_ERR_ARG, "gl_verify: bad circuit description");
    // every count that sizes an allocation below is bounded by what a proof of num_bytes can hold (a description is caller-filled, but a
    // wrong one must be refused, not turned into a 2^40-byte allocation: tools/sanitizer/data_fuzz.cpp)
    GL_REQUIRE(d.num_selectors <= GL_MAX_GATES && d.cap_height <= 16 && d.num_query_rounds <= num_bytes / 8 && d.num_public_inputs <= num_bytes / 8,
               GL_ERR_ARG, check_message(GL_CHECK_DESCRIPTION));
    GL_REQUIRE(!glhost::gate_list_fault(d), GL_ERR_ARG, "gl_verify: bad gate / selector description");
    const size_t nch = 2, R = 80, W = 135, QF = 8, NPP = 9;            // partial products per challenge: ceil(80 / 8) - 1
    s = Shape();
    glopen::Shape& f = s.fri;
    f.hasher = d.hasher; f.num_queries = d.num_query_rounds; f.num_rounds = d.num_fri_rounds; f.cap_height = d.cap_height;
    f.num_oracles = 4; f.num_batches = 2;
    s.lgn = d.degree_bits; f.lgN = s.lgn + d.rate_bits;
    f.ncap = size_t(1) << d.cap_height; s.num_constants = d.num_constants; s.num_public_inputs = d.num_public_inputs;
    unsigned total_arity = 0;
    for (unsigned r = 0; r < d.num_fri_rounds; r++) {
        GL_REQUIRE(d.fri_arity_bits[r] >= 1 && d.fri_arity_bits[r] <= 8, GL_ERR_ARG, "gl_verify: bad FRI arity");
        total_arity += d.fri_arity_bits[r]; f.arity_bits[r] = d.fri_arity_bits[r];
    }
    GL_REQUIRE(total_arity <= s.lgn, GL_ERR_ARG, "gl_verify: FRI reduces below the final polynomial");
    f.final_len = size_t(1) << (s.lgn - total_arity);
    s.nlp = d.num_lookup_polys;                                         // lookup polynomials per challenge, behind Z and the partial products
    // the circuit's instance (fri_instance.hpp).  hiding: the leaves of its blinded oracles -- the wires, Z / partial-products and quotient
    // trees -- end in SALT_SIZE = 4 salt elements (mod.rs:431-456)
    const glfri::PlonkInstance plonk(d);
    size_t leaf_lens[4];
    for (uint32_t o = 0; o < 4; o++) leaf_lens[o] = plonk.inst.oracle_num_polys[o] + (d.zero_knowledge && plonk.inst.oracle_blinding[o] ? glfri::SALT_SIZE : 0);
    // the table in wire order (util/serialization/mod.rs:1939-1981; OpeningSet mod.rs:1409-1423: the lookup vectors sit between zs_next
    // and the partial products), the FriProof behind the openings
    size_t at = 0;
    auto take = [&](size_t k) { const size_t here = at; at = sat_add(at, k); return here; };
    s.o_caps = take(3 * 4 * f.ncap);
    s.o_const = take(2 * s.num_constants); s.o_sig = take(2 * R); s.o_wires = take(2 * W); s.o_zs = take(2 * nch); s.o_zsn = take(2 * nch);
    s.o_lk = take(2 * nch * s.nlp); s.o_lkn = take(2 * nch * s.nlp); s.o_pp = take(2 * nch * NPP); s.o_quot = take(2 * nch * QF);
    glopen::lay_out(f, leaf_lens, plonk.inst.batch_len, plonk.polys.data(), at);
    s.o_pis = f.t_words;
    s.t_words = sat_add(s.o_pis, d.num_public_inputs);
    return GL_OK;
}

int glverify::host_stage(const gl_circuit_desc& d, const Shape& s, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                         const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, glopen::Challenges& ch, uint32_t* check) {
    const size_t nch = 2, R = 80, W = 135, QF = 8, NPP = 9;
    const glopen::Shape& f = s.fri;
    const size_t ncap = f.ncap, NLP = s.nlp;
    const unsigned lgn = s.lgn;
    const size_t n = size_t(1) << lgn;
    *check = GL_CHECK_ACCEPTED;

    // ---- decode (util/serialization/mod.rs:1939-1981 read side, plonk/validate_shape.rs, fri/validate_shape.rs) ----
    const uint32_t hasher = d.hasher;
    Reader rd(proof_bytes, num_bytes, hasher, T);
    // the verifier data's own hashes arrive in four-word slots
    if (!glhost::hashes_well_formed(hasher, constants_sigmas_cap, ncap) || !glhost::hashes_well_formed(hasher, circuit_digest, 1))
        return reject(GL_CHECK_VERIFIER_DATA, check);
    const size_t o_caps = rd.hashes(3 * ncap);
    // OpeningSet in wire order (mod.rs:1409-1423): the lookup vectors sit between zs_next and the partial products
    const size_t o_const = rd.words(2 * d.num_constants), o_sig = rd.words(2 * R), o_wires = rd.words(2 * W), o_zs = rd.words(2 * nch), o_zsn = rd.words(2 * nch),
                 o_lk = rd.words(2 * nch * NLP), o_lkn = rd.words(2 * nch * NLP), o_pp = rd.words(2 * nch * NPP), o_quot = rd.words(2 * nch * QF);
    const size_t o_fcaps = T.size();
    if (const uint32_t bad = decode_fri_proof(rd, f)) return reject(bad, check);
    const gl_t pow_witness = gl_canon(rd.in.u64());
    const uint64_t npis = rd.in.u64();
    if (!rd.in.ok) return reject(GL_CHECK_TRUNCATED, check);
    if (npis != d.num_public_inputs) return reject(GL_CHECK_PUBLIC_INPUT_COUNT, check);
    const size_t o_pis = rd.words(npis);
    if (!rd.in.ok || rd.in.pos != num_bytes) return reject(GL_CHECK_LENGTH, check);
    // every path has the length the description gives it, so the table lies where the shape says (what the queries index by).  The
    // FriProof's own places are not compared one by one: decode_fri_proof walks the shape's counts, so its end says all of them
    GL_REQUIRE(f.paths_fit && T.size() == s.t_words && o_caps == s.o_caps && o_const == s.o_const && o_sig == s.o_sig && o_wires == s.o_wires &&
               o_zs == s.o_zs && o_zsn == s.o_zsn && o_lk == s.o_lk && o_lkn == s.o_lkn && o_pp == s.o_pp && o_quot == s.o_quot &&
               o_fcaps == f.o_fcaps && o_pis == s.o_pis,
               GL_ERR_INTERNAL, "gl_verify: the decoded proof does not lie where its description puts it");
    auto ext_at = [&](size_t off, size_t i) { return gl2_make(T[off + 2 * i], T[off + 2 * i + 1]); };

    // ---- challenges (plonk/get_challenges.rs:26-87, fri/challenges.rs:24-64) ----
    gl_t pi_hash[4];
    glhost::host_hash_no_pad(T.data() + o_pis, npis, pi_hash);
    glhost::HostChallenger tr(hasher);
    tr.observe_hashes(hasher, circuit_digest, 1); tr.observe_many(pi_hash, 4); tr.observe_hashes(hasher, &T[o_caps], ncap);
    gl_t betas[2], gammas[2], alphas[2];
    for (auto& b : betas) b = tr.challenge();
    for (auto& g : gammas) g = tr.challenge();
    // lookup coins (get_challenges.rs:51-63): [betas | gammas | 4 more], four per challenge
    gl_t deltas[8] = {betas[0], betas[1], gammas[0], gammas[1], 0, 0, 0, 0};
    if (NLP) for (int i = 4; i < 8; i++) deltas[i] = tr.challenge();
    tr.observe_hashes(hasher, &T[o_caps + 4 * ncap], ncap);
    for (auto& a : alphas) a = tr.challenge();
    tr.observe_hashes(hasher, &T[o_caps + 8 * ncap], ncap);
    const E zeta = tr.challenge_ext();
    // FriOpenings (plonk/proof.rs:346-380) in the instance's batch order, which is also the order the transcript observes them in:
    // constants, sigmas, wires, zs, partial products, quotient, lookups at zeta; zs_next, lookups_next at g zeta
    std::vector<gl_t> opened;
    opened.reserve(o_fcaps - o_const);
    auto put = [&](size_t off, size_t count) { opened.insert(opened.end(), T.data() + off, T.data() + off + 2 * count); };
    put(o_const, d.num_constants); put(o_sig, R); put(o_wires, W); put(o_zs, nch); put(o_pp, nch * NPP); put(o_quot, nch * QF); put(o_lk, nch * NLP);
    put(o_zsn, nch); put(o_lkn, nch * NLP);
    tr.observe_many(opened.data(), opened.size());
    const gl_t pow_response = draw_fri_challenges(tr, f, T.data(), pow_witness, ch);

    // ---- vanishing(zeta) == Z_H(zeta) * t(zeta) per challenge (plonk/verifier.rs:64-101, vanishing_poly.rs:54-160) ----
    {
        std::vector<E> consts(d.num_constants), wires(W);
        for (size_t i = 0; i < d.num_constants; i++) consts[i] = ext_at(o_const, i);
        for (size_t i = 0; i < W; i++) wires[i] = ext_at(o_wires, i);
        const E zeta_n = e_pow2k(zeta, lgn), z_h = e_sub(zeta_n, e_of(1));
        // L_0(zeta) = (zeta^n - 1) / (n (zeta - 1))  (plonk_common.rs:61-71)
        const E l0 = e_eq(zeta, e_of(1)) ? e_of(1) : e_mul(z_h, gl2_inv(e_scale(e_sub(zeta, e_of(1)), (gl_t)n)));
        // gate constraints, summed slot-wise with each gate's selector filter (vanishing_poly.rs:671-699, gate.rs:277-284)
        std::vector<E> gate_terms(GL_MAX_GATE_CONSTRAINTS, e_of(0));
        const E* gate_consts = consts.data() + d.num_selectors + d.num_lookup_selectors;      // gate.rs:129-133
        E tmp[GL_MAX_GATE_CONSTRAINTS];
        for (unsigned g = 0; g < d.num_gates; g++) {
            const E sel = consts[d.gate_selector_index[g]];
            E filter = e_of(1);
            for (unsigned i = d.gate_group_start[g]; i < d.gate_group_end[g]; i++) if (i != g) filter = e_mul(filter, e_sub(e_of(i), sel));
            if (d.num_selectors > 1) filter = e_mul(filter, e_sub(e_of(glhost::UNUSED_SELECTOR), sel));
            const size_t cnt = gate_constraints_at(d.gate_types[g], d.gate_params[g], wires.data(), gate_consts, pi_hash, tmp);
            // the function and the table are two statements of one fact
            GL_REQUIRE(cnt == glhost::gate_num_constraints(d.gate_types[g], d.gate_params[g]), GL_ERR_INTERNAL, "gl_verify: a gate's constraint count differs from its row of the gate table");
            for (size_t j = 0; j < cnt; j++) gate_terms[j] = e_add(gate_terms[j], e_mul(filter, tmp[j]));
        }
        for (size_t c = 0; c < nch; c++) {
            // terms in the order of vanishing_poly.rs:141-147: all L_0 (Z - 1), all partial-product checks, gate constraints
            std::vector<E> terms;
            for (size_t i = 0; i < nch; i++) terms.push_back(e_mul(l0, e_sub(ext_at(o_zs, i), e_of(1))));
            for (size_t i = 0; i < nch; i++) {
                E num[80], den[80];
                for (size_t j = 0; j < R; j++) {
                    const E wj = wires[j];
                    num[j] = e_add(e_add(wj, e_scale(e_scale(zeta, d.k_is[j]), betas[i])), e_of(gammas[i]));
                    den[j] = e_add(e_add(wj, e_scale(ext_at(o_sig, j), betas[i])), e_of(gammas[i]));
                }
                // check_partial_products (util/partial_products.rs:52-76): chunks of quotient_degree_factor wires
                const size_t chunks = R / QF;
                for (size_t k = 0; k < chunks; k++) {
                    const E prev = k == 0 ? ext_at(o_zs, i) : ext_at(o_pp, i * NPP + k - 1);
                    const E next = k == chunks - 1 ? ext_at(o_zsn, i) : ext_at(o_pp, i * NPP + k);
                    E np = e_of(1), dp = e_of(1);
                    for (size_t j = k * QF; j < (k + 1) * QF; j++) { np = e_mul(np, num[j]); dp = e_mul(dp, den[j]); }
                    terms.push_back(e_sub(e_mul(prev, np), e_mul(next, dp)));
                }
            }
            // lookup constraints of every challenge (vanishing_poly.rs:263-281, 337-500)
            for (size_t i = 0; i < nch && NLP; i++) {
                const gl_t* dl = deltas + glhost::NUM_COINS_LOOKUP * i;
                const size_t num_sldc = NLP - 1, lu_degree = QF - 1, lut_degree = (glhost::LOOKUP_TABLE_SLOTS + num_sldc - 1) / num_sldc;
                const E* sel = consts.data() + d.num_selectors;
                auto zx = [&](size_t k) { return ext_at(o_lk, i * NLP + 1 + k); };
                auto zgx = [&](size_t k) { return ext_at(o_lkn, i * NLP + 1 + k); };
                const E z_re = ext_at(o_lk, i * NLP), next_z_re = ext_at(o_lkn, i * NLP);
                E looked[glhost::LOOKUP_TABLE_SLOTS], combo[glhost::LOOKUP_TABLE_SLOTS], looking[glhost::LOOKUP_SLOTS];
                for (int sl = 0; sl < glhost::LOOKUP_TABLE_SLOTS; sl++) {
                    looked[sl] = e_add(wires[3 * sl], e_scale(wires[3 * sl + 1], dl[glhost::LU_CH_A]));
                    combo[sl] = e_add(wires[3 * sl], e_scale(wires[3 * sl + 1], dl[glhost::LU_CH_B]));
                }
                for (int sl = 0; sl < glhost::LOOKUP_SLOTS; sl++) looking[sl] = e_add(wires[2 * sl], e_scale(wires[2 * sl + 1], dl[glhost::LU_CH_A]));
                terms.push_back(e_mul(sel[glhost::LU_SEL_LAST_LDC], zx(num_sldc - 1)));
                terms.push_back(e_mul(sel[glhost::LU_SEL_INIT_SRE], zx(0)));
                terms.push_back(e_mul(sel[glhost::LU_SEL_INIT_SRE], z_re));
                // final RE, one per table: the table's polynomial at delta (get_lut_poly, vanishing_poly.rs:31-49), on the table's end selector
                for (unsigned t = 0; t < d.num_luts; t++)
                    terms.push_back(e_mul(sel[glhost::LU_SEL_START_END + t], e_sub(z_re, e_of(glhost::lut_poly_at_delta(d, t, dl[glhost::LU_CH_B], dl[glhost::LU_CH_DELTA])))));
                E cur = next_z_re;
                for (int sl = 0; sl < glhost::LOOKUP_TABLE_SLOTS; sl++) cur = e_add(e_scale(cur, dl[glhost::LU_CH_DELTA]), combo[sl]);
                terms.push_back(e_mul(sel[glhost::LU_SEL_TRANS_SRE], e_sub(z_re, cur)));
                const E al = e_of(dl[glhost::LU_CH_ALPHA]);
                for (size_t poly = 0; poly < num_sldc; poly++) {
                    const size_t t0 = poly * lut_degree, t1 = std::min<size_t>((poly + 1) * lut_degree, glhost::LOOKUP_TABLE_SLOTS);
                    const size_t u0 = poly * lu_degree, u1 = std::min<size_t>((poly + 1) * lu_degree, glhost::LOOKUP_SLOTS);
                    E lut_prod = e_of(1), lu_prod = e_of(1), lu_sum = e_of(0), lut_sum_mul = e_of(0);
                    for (size_t a = t0; a < t1; a++) lut_prod = e_mul(lut_prod, e_sub(al, looked[a]));
                    for (size_t a = u0; a < u1; a++) lu_prod = e_mul(lu_prod, e_sub(al, looking[a]));
                    for (size_t a = u0; a < u1; a++) { E pr = e_of(1); for (size_t b = u0; b < u1; b++) if (b != a) pr = e_mul(pr, e_sub(al, looking[b])); lu_sum = e_add(lu_sum, pr); }
                    for (size_t a = t0; a < t1; a++) { E pr = e_of(1); for (size_t b = t0; b < t1; b++) if (b != a) pr = e_mul(pr, e_sub(al, looked[b])); lut_sum_mul = e_add(lut_sum_mul, e_mul(wires[3 * a + 2], pr)); }
                    const E prev = poly == 0 ? zgx(num_sldc - 1) : zx(poly - 1);
                    terms.push_back(e_mul(sel[glhost::LU_SEL_TRANS_SRE], e_sub(e_mul(lut_prod, e_sub(zx(poly), prev)), lut_sum_mul)));
                    terms.push_back(e_mul(sel[glhost::LU_SEL_TRANS_LDC], e_add(e_mul(lu_prod, e_sub(zx(poly), prev)), lu_sum)));
                }
            }
            terms.insert(terms.end(), gate_terms.begin(), gate_terms.end());
            E acc = e_of(0);                                                      // reduce_with_powers (plonk_common.rs:97-128)
            for (size_t t = terms.size(); t-- > 0;) acc = e_add(terms[t], e_scale(acc, alphas[c]));
            E tz = e_of(0);
            for (size_t k = QF; k-- > 0;) tz = e_add(e_mul(tz, zeta_n), ext_at(o_quot, c * QF + k));
            if (!e_eq(acc, e_mul(z_h, tz))) return reject(GL_CHECK_VANISHING, check);
        }
    }

    // ---- FRI (fri/verifier.rs:62-260): the proof of work, and what every query needs ----
    if (!pow_holds(pow_response, d.proof_of_work_bits)) return reject(GL_CHECK_POW, check);
    const E gzeta = e_scale(zeta, glhost::root_of_unity(lgn));
    const uint64_t points[2][2] = {{zeta.a, zeta.b}, {gzeta.a, gzeta.b}};
    reduce_openings(f, opened.data(), points, ch);
    return GL_OK;
}

extern "C" const char* gl_verify_check_message(uint32_t check) noexcept { return glverify::check_message(check); }

extern "C" int gl_verify(const gl_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                         const uint8_t* proof_bytes, size_t num_bytes) try {
    GL_REQUIRE(desc && constants_sigmas_cap && circuit_digest && proof_bytes, GL_ERR_ARG, "gl_verify: null argument");
    const gl_circuit_desc& d = *desc;
    glverify::Shape s;
    GL_TRY(glverify::shape_of(d, num_bytes, s));
    std::vector<gl_t> T;
    glopen::Challenges ch;
    uint32_t check;
    GL_TRY(glverify::host_stage(d, s, constants_sigmas_cap, circuit_digest, proof_bytes, num_bytes, T, ch, &check));
    const gl_t* caps[4] = {constants_sigmas_cap, &T[s.o_caps], &T[s.o_caps + 4 * s.fri.ncap], &T[s.o_caps + 8 * s.fri.ncap]};
    return verify_fri_queries(s.fri, T.data(), ch, caps, nullptr);
} catch (...) { return gl_caught(); }

// convenience for callers that hold the host circuit: CircuitData::verify (plonk/circuit_data.rs:153-155)
extern "C" int gl_host_circuit_verify(const gl_host_circuit* hc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                                      const uint8_t* proof_bytes, size_t num_bytes) try {
    GL_REQUIRE(hc, GL_ERR_ARG, "gl_host_circuit_verify: null circuit");
    return gl_verify(&hc->hc.desc, constants_sigmas_cap, circuit_digest, proof_bytes, num_bytes);
} catch (...) { return gl_caught(); }

// ---- verify_fri_proof for any FriInstanceInfo: the FriProof alone, on the caller's Challenger ----
int glopen::shape_of(const gl_fri_params* params, const gl_fri_instance* instance, Shape& s) {
    GL_TRY(glfri::check(params, instance, false));
    const gl_fri_params& p = *params; const gl_fri_instance& in = *instance;
    s = Shape();
    s.hasher = p.hasher; s.num_queries = p.num_query_rounds; s.num_rounds = p.num_fri_rounds; s.num_oracles = in.num_oracles; s.num_batches = in.num_batches;
    s.cap_height = p.cap_height; s.lgN = p.degree_bits + p.rate_bits;
    s.ncap = size_t(1) << p.cap_height;
    s.final_len = size_t(1) << p.degree_bits;
    for (unsigned r = 0; r < p.num_fri_rounds; r++) { s.arity_bits[r] = p.fri_arity_bits[r]; s.final_len >>= p.fri_arity_bits[r]; }
    size_t leaf_lens[GL_MAX_FRI_ORACLES];
    for (uint32_t o = 0; o < in.num_oracles; o++) leaf_lens[o] = (size_t)in.oracle_num_polys[o] + glfri::salt_of(p, in, o);
    lay_out(s, leaf_lens, in.batch_len, in.polys, 0);             // (glfri::check: the reductions stay above the cap)
    return GL_OK;
}

int glopen::host_stage(const gl_fri_params& p, const gl_fri_instance& in, const Shape& s, const uint64_t (*points)[2], const uint64_t* caps,
                       const uint64_t* openings, gl_challenger* challenger, const uint8_t* proof_bytes, size_t num_bytes, std::vector<gl_t>& T, Challenges& ch,
                       uint32_t* check) {
    if (check) *check = GL_CHECK_ACCEPTED;
    GL_REQUIRE(points, GL_ERR_ARG, "gl_verify_openings: null argument");
    GL_TRY(glfri::check_points(p, in.num_batches, points));
    GL_REQUIRE(caps && openings && challenger && proof_bytes, GL_ERR_ARG, "gl_verify_openings: null argument");
    GL_REQUIRE(challenger->ch.hasher == p.hasher, GL_ERR_ARG, "gl_verify_openings: the challenger runs under another hasher than the params'");
    if (!glhost::hashes_well_formed(p.hasher, caps, in.num_oracles * s.ncap)) return reject(GL_CHECK_VERIFIER_DATA, check);
    Reader rd(proof_bytes, num_bytes, p.hasher, T);
    if (const uint32_t bad = decode_fri_proof(rd, s)) return reject(bad, check);
    const gl_t pow_witness = gl_canon(rd.in.u64());
    if (!rd.in.ok) return reject(GL_CHECK_TRUNCATED, check);
    if (rd.in.pos != num_bytes) return reject(GL_CHECK_LENGTH, check);
    // every path has the length the params give it, and the decode walked the shape's own counts from word 0: the table's end says
    // that every place inside it is where the shape puts it (what the queries index by)
    GL_REQUIRE(T.size() == s.t_words, GL_ERR_INTERNAL, "gl_verify_openings: the decoded proof does not lie where its shape puts it");
    if (!pow_holds(draw_fri_challenges(challenger->ch, s, T.data(), pow_witness, ch), p.proof_of_work_bits)) return reject(GL_CHECK_POW, check);
    reduce_openings(s, openings, points, ch);
    return GL_OK;
}

extern "C" int gl_verify_openings(const gl_fri_params* params, const gl_fri_instance* instance, const uint64_t* caps, const uint64_t* openings,
                                  gl_challenger* challenger, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check) try {
    if (check) *check = GL_CHECK_ACCEPTED;
    glopen::Shape s;
    GL_TRY(glopen::shape_of(params, instance, s));
    std::vector<gl_t> T;
    glopen::Challenges ch;
    GL_TRY(glopen::host_stage(*params, *instance, s, instance->points, caps, openings, challenger, proof_bytes, num_bytes, T, ch, check));
    const gl_t* cap_of[GL_MAX_FRI_ORACLES];
    for (uint32_t o = 0; o < s.num_oracles; o++) cap_of[o] = caps + (size_t)o * 4 * s.ncap;
    return verify_fri_queries(s, T.data(), ch, cap_of, check);
} catch (...) { return gl_caught(); }
