// prove(): host driver replicating the phase order and Fiat-Shamir transcript of plonky2/src/plonk/prover.rs:102-329
// with every polynomial-sized object resident in HBM.  The host sees only Merkle caps, openings, the final FRI
// polynomial, the PoW witness and the query answers; each of those is a mandatory sync point because the next
// phase's challenge is a Poseidon transcript of it (iop/challenger.rs:81-148).
#include "context.hpp"
#include "host_circuit.hpp"
#include "fri_instance.hpp"
#include "prover_kernels.cuh"
#include "proof.hpp"
#include <cstring>
#include <memory>

using glhost::HostChallenger;
using glhost::HostCircuit;

// The context's 1 MiB device staging area (gl_ctx::dev_small), in words, as this file slices it
static constexpr size_t DS_BYTES = size_t(1) << 20, DS_WORDS = DS_BYTES / sizeof(gl_t);
static constexpr size_t DS_APOW = 0, DS_APOW_WORDS = 2 * GLQ_MAX_TERMS;            // quotient: alpha^t per challenge
static constexpr size_t DS_ZH = DS_APOW + DS_APOW_WORDS, DS_ZH_WORDS = 8;          // build(): Z_H on the coset, for L_0
static constexpr size_t DS_POW = DS_ZH + DS_ZH_WORDS, DS_POW_WORDS = 1;            // proof-of-work result
static constexpr size_t DS_OPEN = 4096, DS_OPEN_MAX = 4096, DS_OPEN_WORDS = 2 * DS_OPEN_MAX;   // openings: <= 4096 extension values
static_assert(DS_POW + DS_POW_WORDS <= DS_OPEN && DS_OPEN + DS_OPEN_WORDS <= DS_WORDS, "dev_small slices overlap or do not fit");

struct gl_circuit {
    gl_ctx* ctx = nullptr;
    gl_circuit_desc desc;
    size_t n = 0;
    gl_batch* cs_batch = nullptr;     // constants || sigmas commitment
    gl_t* d_sigmas = nullptr;         // sigma VALUES [80][n]
    gl_t* d_l0_coset = nullptr;       // L_0 on the LDE coset [8n]
    gl_t circuit_digest[4];
    std::unique_ptr<const glfri::PlonkInstance> plonk;      // the FRI instance of every proof of it, but for the two points
};


// ---- device circuit -------------------------------------------------------------------------------------------------
static int validate_desc(const gl_circuit_desc& d) {
    GL_REQUIRE(d.num_wires == 135 && d.num_routed_wires == 80 && d.num_challenges == 2 && d.quotient_degree_factor == 8, GL_ERR_UNSUPPORTED,
               "only standard_recursion_config (135 wires, 80 routed, 2 challenges, quotient factor 8) is supported");
    GL_REQUIRE(d.rate_bits == 3, GL_ERR_UNSUPPORTED, "rate_bits must equal log2(quotient_degree_factor) = 3 (prover.rs:596-608 step = 1)");
    GL_REQUIRE(d.cap_height <= d.degree_bits + d.rate_bits && d.degree_bits >= 1 && d.degree_bits + d.rate_bits <= 24, GL_ERR_ARG, "bad degree / cap height");
    GL_REQUIRE(d.num_gates >= 1 && d.num_gates <= GL_MAX_GATES && d.num_selectors >= 1 && d.num_selectors <= 4, GL_ERR_ARG, "bad gate / selector count");
    { const char* why = glhost::lookup_shape_error(d); GL_REQUIRE(!why, GL_ERR_UNSUPPORTED, why); }
    const uint32_t nrows = 1u << d.degree_bits;
    for (unsigned t = 0; t < d.num_luts; t++)
        GL_REQUIRE(d.last_lu_row[t] < d.last_lut_row[t] && d.last_lut_row[t] <= d.first_lut_row[t] && d.first_lut_row[t] + 1 < nrows &&
                   d.first_lut_row[t] - d.last_lut_row[t] + 1 == glhost::lut_rows(d, t) && (t == 0 || d.last_lu_row[t] > d.first_lut_row[t - 1] + 1),
                   GL_ERR_ARG, "bad lookup rows");
    GL_REQUIRE(d.num_constants == d.num_selectors + d.num_lookup_selectors + 2, GL_ERR_ARG, "bad gate / selector description");
    GL_REQUIRE(d.num_fri_rounds <= 8 && d.num_query_rounds >= 1 && d.num_query_rounds <= 256 && d.proof_of_work_bits <= 40, GL_ERR_ARG, "bad FRI parameters");
    unsigned tot = 0;
    for (unsigned r = 0; r < d.num_fri_rounds; r++) { GL_REQUIRE(d.fri_arity_bits[r] == 4, GL_ERR_UNSUPPORTED, "FRI arity must be 16"); tot += 4; }
    GL_REQUIRE(tot <= d.degree_bits && d.degree_bits + d.rate_bits >= tot + d.cap_height, GL_ERR_ARG, "FRI total reduction arity is too large");   // circuit_builder.rs:977-980
    const glhost::GateListFault fault = glhost::gate_list_fault(d);
    GL_REQUIRE(fault != glhost::GATE_LIST_BAD_TYPE, GL_ERR_UNSUPPORTED, "gate type not in " GL_GATE_LIST);
    GL_REQUIRE(fault != glhost::GATE_LIST_BAD_SELECTOR, GL_ERR_ARG, "bad selector group");
    GL_REQUIRE(d.zero_knowledge <= 1, GL_ERR_ARG, "zero_knowledge is 0 or 1");
    GL_REQUIRE(d.hasher <= GL_HASHER_KECCAK, GL_ERR_ARG, "hasher is 0 (Poseidon) or 1 (Keccak)");
    GL_REQUIRE(!d.zero_knowledge || !d.num_luts, GL_ERR_UNSUPPORTED, "zero knowledge together with lookups is not supported");
    if (d.num_gate_rows) {
        const glhost::BlindingCounts b = glhost::blinding_counts(d.num_gate_rows, d.zero_knowledge, d.rate_bits, d.cap_height, d.num_query_rounds);
        GL_REQUIRE(b.degree_bits == d.degree_bits, GL_ERR_ARG, "degree_bits is not the length blind_and_pad gives num_gate_rows");
    }
    return GL_OK;
}

extern "C" void gl_circuit_free(gl_circuit* c) noexcept {
    if (!c) return;
    if (c->cs_batch) gl_batch_free(c->cs_batch);
    if (c->d_sigmas) c->ctx->pool_release(c->d_sigmas);
    if (c->d_l0_coset) c->ctx->pool_release(c->d_l0_coset);
    gl_ctx_release(c->ctx);
    delete c;
}

// The lookup rows of a description are ProverOnlyCircuitData (lookup_rows, circuit_data.rs:335-360): CommonCircuitData's bytes do not carry
// last_lu_row.  The lookup SELECTOR columns do (gates/selectors.rs:50-103): table t's end selector is 1 at last_lut_row[t] only; LastLdc is 1
// at every table's last_lu_row and InitSre at every first_lut_row + 1, and a table's rows lie between the previous table's and the next
// one's.  build() reads the rows from there and refuses a description that disagrees.
static int lookup_rows_from_selectors(gl_circuit_desc& d, const uint64_t* h_constants) {
    if (!d.num_luts) return GL_OK;
    { const char* why = glhost::lookup_shape_error(d); GL_REQUIRE(!why, GL_ERR_UNSUPPORTED, why); }
    GL_REQUIRE(d.num_constants >= d.num_selectors + d.num_lookup_selectors, GL_ERR_ARG, "bad gate / selector description");
    const size_t n = size_t(1) << d.degree_bits;
    auto ones = [&](unsigned sel, std::vector<uint32_t>& rows) {            // the rows where a 0/1 selector column is 1, ascending
        const uint64_t* col = h_constants + (size_t)(d.num_selectors + sel) * n;
        for (size_t r = 0; r < n; r++) if (col[r] == 1) rows.push_back((uint32_t)r); else if (col[r] != 0) return false;
        return true;
    };
    std::vector<uint32_t> last_ldc, init_sre;
    GL_REQUIRE(ones(glhost::LU_SEL_LAST_LDC, last_ldc) && ones(glhost::LU_SEL_INIT_SRE, init_sre) && last_ldc.size() == d.num_luts && init_sre.size() == d.num_luts,
               GL_ERR_ARG, "lookup selector columns do not describe num_luts tables");
    for (unsigned t = 0; t < d.num_luts; t++) {
        std::vector<uint32_t> end;
        GL_REQUIRE(ones(glhost::LU_SEL_START_END + t, end) && end.size() == 1, GL_ERR_ARG, "a table's end selector must be 1 on exactly one row");
        // tables are placed in order (gadgets/lookup.rs:79-125): the t-th LastLdc / InitSre rows are table t's
        const uint32_t lu = last_ldc[t], lut = end[0], first = init_sre[t] - 1;
        GL_REQUIRE(init_sre[t] >= 1 && lu < lut && lut <= first, GL_ERR_ARG, "lookup selector columns do not describe the tables in order");
        // a description read from common-data bytes has last_lu_row = 0 (unknown); any row it does name has to agree
        GL_REQUIRE((!d.last_lu_row[t] || d.last_lu_row[t] == lu) && (!d.last_lut_row[t] || d.last_lut_row[t] == lut) && (!d.first_lut_row[t] || d.first_lut_row[t] == first),
                   GL_ERR_ARG, "the description's lookup rows disagree with the lookup selector columns");
        d.last_lu_row[t] = lu; d.last_lut_row[t] = lut; d.first_lut_row[t] = first;
    }
    return GL_OK;
}

int gl_sigmas_from_classes(gl_ctx* c, const uint64_t* d_classes, uint32_t lgn, uint32_t ncols, const uint64_t* h_k_is, gl_t* d_sigma);      // sigma.hip

// Z_H = X^n - 1 on the LDE coset 7 H_N, which takes the 8 values (7 w_8^i)^n - 1 (ZeroPolyOnCoset, field/src/zero_poly_coset.rs:19-36)
static void zh_on_coset(const gl_circuit_desc& d, gl_t zh[8]) {
    gl_t g_pow_n = GL_MULT_GENERATOR; for (uint32_t i = 0; i < d.degree_bits; i++) g_pow_n = gl_sqr(g_pow_n);
    gl_t w8 = gl_host_root_of_unity(d.rate_bits), x = 1;
    for (int i = 0; i < 8; i++) { zh[i] = gl_canon(gl_sub(gl_mul(g_pow_n, x), 1)); x = gl_mul(x, w8); }
}

// the rest of the device half of build() once the constants || sigmas VALUE columns are in HBM (d_cs[num_constants + 80][n])
static int circuit_finish(gl_ctx* ctx, const gl_circuit_desc* desc, const gl_t* d_cs, gl_circuit** out) {
    std::unique_ptr<gl_circuit, void (*)(gl_circuit*)> c(new gl_circuit(), gl_circuit_free);
    c->ctx = ctx; ctx->retain(); c->desc = *desc; c->n = size_t(1) << desc->degree_bits;
    c->plonk.reset(new glfri::PlonkInstance(*desc));
    const size_t n = c->n, ncs = desc->num_constants + 80;
    GL_TRY(gl_batch_from_device_h(ctx, desc->hasher, d_cs, ncs, n, desc->rate_bits, desc->cap_height, 1, &c->cs_batch));      // circuit_builder.rs:1020-1028
    GL_TRY(ctx->pool_alloc(80 * n * sizeof(gl_t), (void**)&c->d_sigmas));
    GL_CHECK_HIP(hipMemcpyAsync(c->d_sigmas, d_cs + (size_t)desc->num_constants * n, 80 * n * sizeof(gl_t), hipMemcpyDeviceToDevice, ctx->stream));
    {   // L_0 on the coset 7 H_N, N = n << rate_bits
        const uint32_t lgN = desc->degree_bits + desc->rate_bits;
        const size_t N = size_t(1) << lgN;
        GL_TRY(ctx->pool_alloc(N * sizeof(gl_t), (void**)&c->d_l0_coset));
        GlPowTable xt;
        GL_TRY(ctx->get_pow_table(gl_host_root_of_unity(lgN), GL_MULT_GENERATOR, (uint32_t)((N + 2047) >> 11), &xt));
        gl_t zh[DS_ZH_WORDS];
        zh_on_coset(*desc, zh);
        GL_TRY(ctx->ensure_dev_small(DS_BYTES));
        gl_t* d_zh = ctx->dev_small + DS_ZH;
        GL_TRY(gl_copy_h2d(ctx, d_zh, zh, sizeof zh));
        hipLaunchKernelGGL(k_l0_on_coset, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, xt.lo, xt.hi, (uint32_t)N, (gl_t)n, d_zh, c->d_l0_coset);
        GL_CHECK_HIP(hipGetLastError());
        GL_CHECK_HIP(gl_stream_wait(ctx->stream));
    }
    // circuit_digest = hash_no_pad(cap || hash_pad([]) || [degree_bits]) under C::Hasher   (circuit_builder.rs:1086-1098)
    std::vector<gl_t> cap((size_t(4) << desc->cap_height));
    GL_TRY(gl_batch_cap(c->cs_batch, cap.data()));
    glhost::circuit_digest(desc->hasher, cap.data(), size_t(1) << desc->cap_height, desc->degree_bits, c->circuit_digest);
    *out = c.release();
    return GL_OK;
}
extern "C" int gl_circuit_create(gl_ctx* ctx, const gl_circuit_desc* desc, const uint64_t* h_cs, gl_circuit** out) try {
    GL_REQUIRE(ctx && desc && h_cs && out, GL_ERR_ARG, "null argument");
    GL_REQUIRE(desc->degree_bits >= 1 && desc->degree_bits <= 21 && desc->num_selectors <= 4, GL_ERR_ARG, "bad degree / selector count");
    gl_circuit_desc d = *desc;
    GL_TRY(lookup_rows_from_selectors(d, h_cs));
    GL_TRY(validate_desc(d));
    GL_TRY(ctx->activate());
    const size_t n = size_t(1) << d.degree_bits, ncs = d.num_constants + 80;
    DevBuf d_cs(ctx); GL_TRY(d_cs.alloc(ncs * n * sizeof(gl_t)));
    GL_TRY(gl_copy_h2d(ctx, d_cs.p, h_cs, ncs * n * sizeof(gl_t)));
    return circuit_finish(ctx, &d, d_cs.as<gl_t>(), out);
} catch (...) { return gl_caught(); }
// build() with the sigma polynomials computed on the device from the copy-constraint classes (sigma.hip)
extern "C" int gl_circuit_create_from_classes(gl_ctx* ctx, const gl_circuit_desc* desc, const uint64_t* h_constants, const uint64_t* h_wire_classes, gl_circuit** out) try {
    GL_REQUIRE(ctx && desc && h_constants && h_wire_classes && out, GL_ERR_ARG, "null argument");
    GL_REQUIRE(desc->degree_bits >= 1 && desc->degree_bits <= 21 && desc->num_selectors <= 4, GL_ERR_ARG, "bad degree / selector count");
    gl_circuit_desc dd = *desc;
    GL_TRY(lookup_rows_from_selectors(dd, h_constants));
    desc = &dd;
    GL_TRY(validate_desc(*desc));
    GL_TRY(ctx->activate());
    const size_t n = size_t(1) << desc->degree_bits, nc = desc->num_constants;
    DevBuf d_cs(ctx), d_cls(ctx);
    GL_TRY(d_cs.alloc((nc + 80) * n * sizeof(gl_t)));
    GL_TRY(d_cls.alloc(80 * n * sizeof(uint64_t)));
    GL_TRY(gl_copy_h2d(ctx, d_cs.p, h_constants, nc * n * sizeof(gl_t)));
    GL_TRY(gl_copy_h2d(ctx, d_cls.p, h_wire_classes, 80 * n * sizeof(uint64_t)));
    ctx->timing_begin("sigma polynomials");
    int st = gl_sigmas_from_classes(ctx, d_cls.as<uint64_t>(), desc->degree_bits, 80, desc->k_is, d_cs.as<gl_t>() + nc * n);
    ctx->timing_end();
    GL_TRY(st);
    return circuit_finish(ctx, desc, d_cs.as<gl_t>(), out);
} catch (...) { return gl_caught(); }
extern "C" int gl_circuit_from_host(gl_ctx* ctx, const gl_host_circuit* hc, gl_circuit** out) try {
    GL_REQUIRE(hc, GL_ERR_ARG, "null host circuit");
    // the constant columns are the first num_constants columns of the host matrix; the sigma columns come from the classes
    return gl_circuit_create_from_classes(ctx, &hc->hc.desc, hc->hc.constants_sigmas.data(), hc->hc.wire_class.data(), out);
} catch (...) { return gl_caught(); }
extern "C" int gl_circuit_description(const gl_circuit* c, gl_circuit_desc* out) try {
    GL_REQUIRE(c && out, GL_ERR_ARG, "null argument");
    *out = c->desc;
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_circuit_digest(const gl_circuit* c, uint64_t h_out[4]) try {
    GL_REQUIRE(c && h_out, GL_ERR_ARG, "null argument");
    memcpy(h_out, c->circuit_digest, 32);
    return GL_OK;
} catch (...) { return gl_caught(); }
extern "C" int gl_circuit_constants_sigmas_cap(const gl_circuit* c, uint64_t* h_out) try {
    GL_REQUIRE(c && h_out, GL_ERR_ARG, "null argument");
    return gl_batch_cap(c->cs_batch, h_out);
} catch (...) { return gl_caught(); }
extern "C" const gl_batch* gl_circuit_constants_sigmas_batch(const gl_circuit* c) noexcept { return c ? c->cs_batch : nullptr; }

// ---- helpers -------------------------------------------------------------------------------------------------------------
static inline gl2_t h_ext(gl_t a, gl_t b) { return gl2_make(a, b); }
// put_u64 / put_words / put_hashes and BatchHolder: proof.hpp, shared with stark.hip
static uint32_t host_bitrev32(uint32_t x, uint32_t bits) { uint32_t r = 0; for (uint32_t i = 0; i < bits; i++) r = (r << 1) | ((x >> i) & 1); return r; }

struct MerkleHolder { gl_ctx* c; GlMerkle m; explicit MerkleHolder(gl_ctx* ctx) : c(ctx) {} ~MerkleHolder() { gl_merkle_release(c, &m); } };

static int d2h(gl_ctx* c, void* dst, const void* src, size_t bytes) { return gl_copy_d2h(c, dst, src, bytes); }
static int h2d_async(gl_ctx* c, void* dst, const void* src, size_t bytes) {
    // sources are small host vectors that outlive the next sync; pageable H2D is staged by the runtime before returning
    GL_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return GL_OK;
}

// Host witness -> HBM through a two-deep ring of pinned chunks (the drop-in entry points gl_prove / gl_prove_columns; reference side:
// MatrixWitness.wire_values, iop/witness.rs:256-258, handed to PolynomialBatch::from_values at plonk/prover.rs:145-156).
// A hipMemcpyAsync from PAGEABLE memory is staged by the runtime inside the call: the calling thread spins there until the
// stream's earlier work is done and the copy is on its way (the round-2 finding for the D2H direction: a full core per proof in
// flight).  Here the host thread copies the columns into one of two pinned chunks (plain memcpy, ~10 GB/s), hands the chunk to
// the copy engine and fills the other one meanwhile; it only ever waits, sleeping between polls, for a chunk to come back.
// The DMA of a proof's witness runs under the kernels of the other proofs in flight on the device's other contexts.
static hipError_t gl_event_wait(hipEvent_t ev) {
    hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(30)) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        } else { struct timespec ts = {0, 20000}; (void)nanosleep(&ts, nullptr); }
    }
}
struct H2dRing {
    gl_ctx* c; void* buf[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0}; hipEvent_t ev[2] = {nullptr, nullptr}; bool busy[2] = {false, false};
    explicit H2dRing(gl_ctx* ctx) : c(ctx) {}
    int init(size_t chunk_bytes) {
        for (int k = 0; k < 2; k++) {
            GL_TRY(c->pin_acquire(chunk_bytes, &buf[k], &cap[k]));
            GL_CHECK_HIP(hipEventCreateWithFlags(&ev[k], hipEventDisableTiming));
        }
        return GL_OK;
    }
    int slot_free(int k) { if (busy[k]) { GL_CHECK_HIP(gl_event_wait(ev[k])); busy[k] = false; } return GL_OK; }
    int send(int k, void* d_dst, size_t bytes) {
        GL_CHECK_HIP(hipMemcpyAsync(d_dst, buf[k], bytes, hipMemcpyHostToDevice, c->stream));
        GL_CHECK_HIP(hipEventRecord(ev[k], c->stream));
        busy[k] = true;
        return GL_OK;
    }
    ~H2dRing() {                  // a chunk goes back to the context's list only after the copy engine has read it
        for (int k = 0; k < 2; k++) {
            if (busy[k]) (void)gl_event_wait(ev[k]);
            if (ev[k]) (void)hipEventDestroy(ev[k]);
            if (buf[k]) c->pin_release(buf[k], cap[k]);
        }
    }
};
static const size_t GL_H2D_CHUNK = size_t(8) << 20;
// cols != null: ncols host vectors of n elements each (d_dst[c * n + i] = cols[c][i]); else `flat`, ncols * n contiguous elements
static int h2d_witness(gl_ctx* ctx, gl_t* d_dst, size_t ncols, size_t n, const uint64_t* const* cols, const uint64_t* flat) {
    const size_t col_bytes = n * sizeof(gl_t), total = ncols * col_bytes;
    if (!total) return GL_OK;
    H2dRing ring(ctx);
    GL_TRY(ring.init(total < GL_H2D_CHUNK ? total : GL_H2D_CHUNK));
    const size_t chunk = ring.cap[0] < ring.cap[1] ? ring.cap[0] : ring.cap[1];
    size_t off = 0; int k = 0;
    while (off < total) {
        const size_t len = total - off < chunk ? total - off : chunk;
        GL_TRY(ring.slot_free(k));
        if (!cols) memcpy(ring.buf[k], (const char*)flat + off, len);
        else {
            size_t done = 0;
            while (done < len) {                        // a chunk may begin and end inside a column
                const size_t c = (off + done) / col_bytes, in_col = (off + done) % col_bytes;
                const size_t piece = (col_bytes - in_col) < (len - done) ? (col_bytes - in_col) : (len - done);
                memcpy((char*)ring.buf[k] + done, (const char*)cols[c] + in_col, piece);
                done += piece;
            }
        }
        GL_TRY(ring.send(k, (char*)d_dst + off, len));
        off += len; k ^= 1;
    }
    return GL_OK;                                       // ~H2dRing waits for the last two chunks (the DMA of <= 16 MiB)
}

// ======================================================================================================================
// Phase-level entry points: the seam of SURVEY 8(b).  A caller that keeps the Fiat-Shamir transcript on its side (the
// reference's Challenger in Rust) drives these one by one; gl_prove() below is exactly that driver with the transcript
// in C++.  Every phase leaves its polynomials in HBM and hands back only what the transcript needs.
// ======================================================================================================================

// the coset shifts of get_unique_coset_shifts (field/src/cosets.rs:9-24) are 1, 7, 7^2, ...: lets the kernels step beta x k_j by x7
static uint32_t k_is_are_powers_of_7(const gl_circuit_desc& d) {
    gl_t x = 1;
    for (int j = 0; j < 80; j++) { if (gl_canon(d.k_is[j]) != x) return 0; x = gl_canon(gl_mul(x, GL_MULT_GENERATOR)); }
    return 1;
}

// ---- 6. all_wires_permutation_partial_products (plonk/prover.rs:332-416): d_zs[20][n] VALUES ----
static int partial_products_values(gl_ctx* ctx, const gl_circuit* cir, const gl_t* d_wires, const gl_t* betas, const gl_t* gammas, gl_t* d_zs) {
    const gl_circuit_desc& d = cir->desc;
    const size_t n = cir->n;
    hipStream_t st = ctx->stream;
    DevBuf d_chunk(ctx), d_rowp(ctx), d_seg(ctx);
    const uint32_t nseg = (uint32_t)((n + GLP_SEG - 1) / GLP_SEG);
    GL_TRY(d_chunk.alloc(2 * GLP_CHUNKS * n * sizeof(gl_t)));
    DevBuf d_den(ctx); GL_TRY(d_den.alloc(2 * GLP_CHUNKS * n * sizeof(gl_t)));
    GL_TRY(d_rowp.alloc(2 * n * sizeof(gl_t)));
    GL_TRY(d_seg.alloc(2 * (size_t)nseg * sizeof(gl_t)));
    GlPowTable xt;
    GL_TRY(ctx->get_pow_table(gl_host_root_of_unity(d.degree_bits), 1, (uint32_t)((n + 2047) >> 11), &xt));
    GlPermParams pp;
    pp.wires = d_wires; pp.sigmas = cir->d_sigmas; pp.xpow_lo = xt.lo; pp.xpow_hi = xt.hi;
    for (int j = 0; j < 80; j++) pp.k_is[j] = d.k_is[j];
    pp.k_is_powers_of_7 = k_is_are_powers_of_7(d);
    for (int i = 0; i < 2; i++) { pp.betas[i] = gl_canon(betas[i]); pp.gammas[i] = gl_canon(gammas[i]); }
    pp.n = (uint32_t)n; pp.chunk_prod = d_chunk.as<gl_t>(); pp.row_prod = d_rowp.as<gl_t>();
    ctx->timing_begin("compute partial products");
    hipLaunchKernelGGL(k_pp_chunk_terms, dim3((unsigned)((n + 255) / 256), 2 * GLP_CHUNKS), dim3(256), 0, st, pp, d_den.as<gl_t>());
    hipLaunchKernelGGL(k_pp_chunk_products, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, st, pp, d_den.as<const gl_t>(), gl_launch_prio(2 * n));
    hipLaunchKernelGGL(k_z_segment_products, dim3(nseg, 2), dim3(256), 0, st, d_rowp.as<gl_t>(), (uint32_t)n, d_seg.as<gl_t>(), gl_launch_prio(512ull * nseg));
    hipLaunchKernelGGL(k_z_segment_scan, dim3(1), dim3(64), 0, st, d_seg.as<gl_t>(), nseg, gl_launch_prio(64));
    hipLaunchKernelGGL(k_z_finalize, dim3(nseg, 2), dim3(256), 0, st, d_rowp.as<gl_t>(), d_chunk.as<gl_t>(), d_seg.as<gl_t>(), (uint32_t)n, d_zs);
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}
// ---- compute_all_lookup_polys (plonk/prover.rs:425-572): d_out[2 * 7][n] VALUES (RE + 6 partial SLDC per challenge) ----
static int lookup_polys_values(gl_ctx* ctx, const gl_circuit* cir, const gl_t* d_wires, const gl_t* deltas8, gl_t* d_out) {
    const gl_circuit_desc& d = cir->desc;
    const size_t n = cir->n;
    hipStream_t st = ctx->stream;
    uint32_t max_rows = 0;
    for (unsigned t = 0; t < d.num_luts; t++) max_rows = std::max(max_rows, d.first_lut_row[t] - d.last_lu_row[t] + 1);
    DevBuf d_agg(ctx); GL_TRY(d_agg.alloc((size_t)2 * max_rows * 8 * sizeof(gl_t)));
    gl_t dl[8]; for (int i = 0; i < 8; i++) dl[i] = gl_canon(deltas8[i]);
    ctx->timing_begin("compute lookup polys");
    GL_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)2 * d.num_lookup_polys * n * sizeof(gl_t), st));
    // the tables share the polynomials and own disjoint row ranges, each starting from zero on the row above its first table row
    // (prover.rs:449-454: one pass per LookupWire); the launches of one table follow the previous table's on the stream
    for (unsigned t = 0; t < d.num_luts; t++) {
        const uint32_t nrows = d.first_lut_row[t] - d.last_lu_row[t] + 1;
        hipLaunchKernelGGL(k_lookup_inverses, dim3(nrows, 2), dim3(64), 0, st, d_wires, (uint32_t)n, d.last_lu_row[t], d.last_lut_row[t],
                           dl[glhost::LU_CH_A], dl[glhost::LU_CH_ALPHA], dl[glhost::LU_CH_B], dl[glhost::LU_CH_DELTA],
                           dl[4 + glhost::LU_CH_A], dl[4 + glhost::LU_CH_ALPHA], dl[4 + glhost::LU_CH_B], dl[4 + glhost::LU_CH_DELTA], d_agg.as<gl_t>());
        hipLaunchKernelGGL(k_lookup_scan, dim3(1), dim3(64), 0, st, (uint32_t)n, d.last_lu_row[t], d.last_lut_row[t], d.first_lut_row[t],
                           dl[glhost::LU_CH_DELTA], dl[4 + glhost::LU_CH_DELTA], d_agg.as<const gl_t>(), d_out);
    }
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}
static int check_phase_args(gl_ctx* ctx, const gl_circuit* cir) {
    GL_REQUIRE(ctx && cir, GL_ERR_ARG, "null context / circuit");
    GL_REQUIRE(cir->ctx->device == ctx->device, GL_ERR_ARG, "circuit lives on another device");
    return ctx->activate();
}
// the phase API commits without salt: a zero-knowledge circuit is proved by gl_prove* only
static int check_phase_api(gl_ctx* ctx, const gl_circuit* cir) {
    GL_TRY(check_phase_args(ctx, cir));
    GL_REQUIRE(!cir->desc.zero_knowledge, GL_ERR_UNSUPPORTED, "the phase API does not prove zero-knowledge circuits (use gl_prove*)");
    return GL_OK;
}
static int check_batch(const gl_circuit* cir, const gl_batch* b, size_t ncols, const char* what) {
    GL_REQUIRE(b && b->ncols == ncols && b->n == cir->n && b->rate_bits == cir->desc.rate_bits && b->cap_height == cir->desc.cap_height, GL_ERR_ARG, what);
    GL_REQUIRE(b->hasher == cir->desc.hasher, GL_ERR_ARG, "a batch committed under another hasher than the circuit's");
    return GL_OK;
}
// Z || partial products (|| lookup polynomials) -> committed batch (prover.rs:189-223), for gl_partial_products[_lookups] and prove().
// `deltas8` is null exactly for a circuit without lookups; `capture`, if given, receives the value columns; `seed`: salt key (zero knowledge) or null.
static int commit_zs(gl_ctx* ctx, const gl_circuit* cir, const gl_t* d_wires, const gl_t* betas, const gl_t* gammas, const gl_t* deltas8,
                     gl_batch** out, std::vector<gl_t>* capture, const uint8_t* seed = nullptr) {
    const size_t n = cir->n, nzs = 20 + 2 * (size_t)cir->desc.num_lookup_polys;
    DevBuf d_zs(ctx); GL_TRY(d_zs.alloc(nzs * n * sizeof(gl_t)));
    GL_TRY(partial_products_values(ctx, cir, d_wires, betas, gammas, d_zs.as<gl_t>()));
    if (deltas8) GL_TRY(lookup_polys_values(ctx, cir, d_wires, deltas8, d_zs.as<gl_t>() + 20 * n));
    if (capture) { capture->resize(nzs * n); GL_TRY(d2h(ctx, capture->data(), d_zs.p, nzs * n * sizeof(gl_t))); }
    return gl_batch_from_device_salted(ctx, d_zs.as<uint64_t>(), nzs, n, cir->desc.rate_bits, cir->desc.cap_height, 1, seed, 2, out, cir->desc.hasher);
}
static int partial_products_phase(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t* betas, const uint64_t* gammas, const uint64_t* deltas8, gl_batch** out) {
    GL_TRY(check_phase_api(ctx, cir));
    GL_REQUIRE(d_wires && betas && gammas && out, GL_ERR_ARG, "gl_partial_products: null argument");
    GL_REQUIRE((cir->desc.num_lookup_polys != 0) == (deltas8 != nullptr), GL_ERR_ARG, "circuits with lookups take gl_partial_products_lookups (with the delta challenges), circuits without take gl_partial_products");
    return commit_zs(ctx, cir, d_wires, betas, gammas, deltas8, out, nullptr);
}
extern "C" int gl_partial_products(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t betas[2], const uint64_t gammas[2], gl_batch** out) try {
    return partial_products_phase(ctx, cir, d_wires, betas, gammas, nullptr, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_partial_products_lookups(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t betas[2], const uint64_t gammas[2],
                                           const uint64_t deltas[8], gl_batch** out) try {
    GL_REQUIRE(deltas, GL_ERR_ARG, "gl_partial_products_lookups: null deltas");
    return partial_products_phase(ctx, cir, d_wires, betas, gammas, deltas, out);
} catch (...) { return gl_caught(); }

// ---- 9/10. compute_quotient_polys + split + commitment (plonk/prover.rs:229-271,574-744), for gl_quotient_polys[_lookups] and prove():
//      d_q[2][8n] -> the 16 chunk COEFFICIENT columns -> committed batch.  `apow` is the host source of an asynchronous upload: the caller
//      keeps it alive up to its next sync.  `deltas8` is null exactly for a circuit without lookups; `capture` receives the chunks. ----
static int commit_quotient(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* wires, const gl_batch* zs, const gl_t* pi_hash, const gl_t* betas,
                           const gl_t* gammas, const gl_t* alphas, const gl_t* deltas8, std::vector<gl_t>& apow, gl_batch** out, std::vector<gl_t>* capture,
                           const uint8_t* seed = nullptr) {
    const gl_circuit_desc& d = cir->desc;
    const size_t n = cir->n, N = n << d.rate_bits;
    const uint32_t lgN = d.degree_bits + d.rate_bits;
    hipStream_t st = ctx->stream;
    DevBuf d_q(ctx); GL_TRY(d_q.alloc(2 * N * sizeof(gl_t)));
    apow.assign(DS_APOW_WORDS, 0);
    for (int b = 0; b < 2; b++) { gl_t x = 1; const gl_t al = gl_canon(alphas[b]); for (int t = 0; t < GLQ_MAX_TERMS; t++) { apow[b * GLQ_MAX_TERMS + t] = x; x = gl_canon(gl_mul(x, al)); } }
    GL_TRY(ctx->ensure_dev_small(DS_BYTES));
    gl_t* d_apow = ctx->dev_small + DS_APOW;
    GL_TRY(h2d_async(ctx, d_apow, apow.data(), apow.size() * sizeof(gl_t)));
    GlPowTable xt;
    GL_TRY(ctx->get_pow_table(gl_host_root_of_unity(lgN), GL_MULT_GENERATOR, (uint32_t)((N + 2047) >> 11), &xt));
    GlQuotParams q;
    ::memset((void*)&q, 0, sizeof q);
    q.cs = cir->cs_batch->lde; q.wires = wires->lde; q.zs = zs->lde; q.xpow_lo = xt.lo; q.xpow_hi = xt.hi;
    q.alpha_pows = d_apow; q.out = d_q.as<gl_t>();
    for (int j = 0; j < 80; j++) q.k_is[j] = d.k_is[j];
    q.k_is_powers_of_7 = k_is_are_powers_of_7(d);
    for (int i = 0; i < 2; i++) { q.betas[i] = gl_canon(betas[i]); q.gammas[i] = gl_canon(gammas[i]); }
    for (int i = 0; i < 4; i++) q.pi_hash[i] = gl_canon(pi_hash[i]);
    zh_on_coset(d, q.zh_evals);
    for (int i = 0; i < 8; i++) q.zh_inv[i] = gl_canon(gl_inv(q.zh_evals[i]));
    q.l0_coset = cir->d_l0_coset;
    q.n_field = (gl_t)n; q.lgN = lgN; q.num_constants = d.num_constants; q.num_selectors = d.num_selectors; q.num_gates = d.num_gates;
    q.next_step = 1u << d.rate_bits;
    q.num_lookup_selectors = d.num_lookup_selectors; q.num_lookup_polys = d.num_lookup_polys;
    q.num_luts = d.num_luts;
    q.gate_term0 = 2 + 2 * GLP_CHUNKS + (d.num_lookup_polys ? 2 * GLQ_LOOKUP_TERMS(d.num_luts) : 0);
    if (d.num_lookup_polys) {
        GL_REQUIRE(deltas8, GL_ERR_ARG, "a circuit with lookups needs the delta challenges");
        for (int i = 0; i < 8; i++) q.deltas[i] = gl_canon(deltas8[i]);
        for (int c = 0; c < 2; c++)
            for (unsigned t = 0; t < d.num_luts; t++)
                q.lut_poly_at_delta[c][t] = glhost::lut_poly_at_delta(d, t, q.deltas[4 * c + glhost::LU_CH_B], q.deltas[4 * c + glhost::LU_CH_DELTA]);
    }
    for (unsigned g = 0; g < d.num_gates; g++) { q.gate_types[g] = d.gate_types[g]; q.gate_params[g] = d.gate_params[g]; q.gate_sel[g] = d.gate_selector_index[g]; q.group_start[g] = d.gate_group_start[g]; q.group_end[g] = d.gate_group_end[g]; }
    ctx->timing_begin("compute quotient polys");
    uint32_t launches = 0;                           // the launch classes (gates.hpp's table) this circuit's gates need
    for (unsigned g = 0; g < d.num_gates; g++) launches |= 1u << glhost::gate_launch(d.gate_types[g]);
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_quotient<false>, grid, block, 0, st, q);      // always: it also writes the Z and partial-product terms
    if ((launches >> glhost::LAUNCH_POSEIDON) & 1) hipLaunchKernelGGL(k_quotient<true>, grid, block, 0, st, q);
    if ((launches >> glhost::LAUNCH_RANDOM_ACCESS) & 1) hipLaunchKernelGGL(k_quotient_random_access, grid, block, 0, st, q);
    if ((launches >> glhost::LAUNCH_EXT_ARITH) & 1) hipLaunchKernelGGL(k_quotient_ext_arith, grid, block, 0, st, q);
    if (d.num_lookup_polys) hipLaunchKernelGGL(k_quotient_lookup, grid, block, 0, st, q);
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    // coset_ifft(7) of each quotient (prover.rs:739-743); the 8n coefficients ARE the 8 chunks of n (prover.rs:245-258)
    GL_TRY(gl_ntt_run(ctx, d_q.as<gl_t>(), N, (uint32_t)N, d_q.as<gl_t>(), N, lgN, 2, true, 0, gl_canon(gl_inv(GL_MULT_GENERATOR)), gl_host_inverse_2exp(lgN)));
    if (capture) { capture->resize(16 * n); GL_TRY(d2h(ctx, capture->data(), d_q.p, 16 * n * sizeof(gl_t))); }
    return gl_batch_from_device_salted(ctx, d_q.as<uint64_t>(), 16, n, d.rate_bits, d.cap_height, 0, seed, 3, out, d.hasher);
}
static int quotient_phase(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* wires, const gl_batch* zs_partial_products, const uint64_t* pi_hash,
                          const uint64_t* betas, const uint64_t* gammas, const uint64_t* alphas, const uint64_t* deltas8, gl_batch** out) {
    GL_TRY(check_phase_api(ctx, cir));
    GL_REQUIRE(pi_hash && betas && gammas && alphas && out, GL_ERR_ARG, "gl_quotient_polys: null argument");
    const size_t nlk = 2 * (size_t)cir->desc.num_lookup_polys;
    GL_REQUIRE((nlk != 0) == (deltas8 != nullptr), GL_ERR_ARG, "circuits with lookups take gl_quotient_polys_lookups (with the delta challenges), circuits without take gl_quotient_polys");
    GL_TRY(check_batch(cir, wires, 135, "gl_quotient_polys: wires batch does not match the circuit"));
    GL_TRY(check_batch(cir, zs_partial_products, 20 + nlk, "gl_quotient_polys: Z / partial-products (/ lookups) batch does not match the circuit"));
    std::vector<gl_t> apow;
    const int rc = commit_quotient(ctx, cir, wires, zs_partial_products, pi_hash, betas, gammas, alphas, deltas8, apow, out, nullptr);
    GL_CHECK_HIP(gl_stream_wait(ctx->stream));      // `apow` was the source of an async upload
    return rc;
}
extern "C" int gl_quotient_polys(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* wires, const gl_batch* zs_partial_products, const uint64_t pi_hash[4],
                                 const uint64_t betas[2], const uint64_t gammas[2], const uint64_t alphas[2], gl_batch** out) try {
    return quotient_phase(ctx, cir, wires, zs_partial_products, pi_hash, betas, gammas, alphas, nullptr, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_quotient_polys_lookups(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* wires, const gl_batch* zs_partial_products_lookups, const uint64_t pi_hash[4],
                                         const uint64_t betas[2], const uint64_t gammas[2], const uint64_t alphas[2], const uint64_t deltas[8], gl_batch** out) try {
    GL_REQUIRE(deltas, GL_ERR_ARG, "gl_quotient_polys_lookups: null deltas");
    return quotient_phase(ctx, cir, wires, zs_partial_products_lookups, pi_hash, betas, gammas, alphas, deltas, out);
} catch (...) { return gl_caught(); }

// ---- 12. OpeningSet::new (plonk/proof.rs:306-344): polynomials `first .. first + count` of a batch at an extension point ----
static void launch_open(gl_ctx* ctx, const gl_batch* b, size_t first, size_t count, gl2_t z, gl_t* d_out) {
    hipLaunchKernelGGL(k_eval_at_ext, dim3((unsigned)count), dim3(256), 0, ctx->stream, b->coeffs + first * b->n, (uint32_t)b->n, (uint64_t)b->n, z.a, z.b, d_out);
}
extern "C" int gl_open_at(gl_ctx* ctx, const gl_batch* b, const uint64_t z[2], size_t first_col, size_t num_cols, uint64_t* h_out) try {
    GL_REQUIRE(ctx && b && z && h_out, GL_ERR_ARG, "gl_open_at: null argument");
    GL_REQUIRE(first_col <= b->ncols && num_cols <= b->ncols - first_col && num_cols <= DS_OPEN_MAX, GL_ERR_ARG, "gl_open_at: column range out of bounds");
    if (!num_cols) return GL_OK;
    GL_TRY(ctx->activate());
    GL_TRY(ctx->ensure_dev_small(DS_BYTES));
    gl_t* d_open = ctx->dev_small + DS_OPEN;
    ctx->timing_begin("construct the opening set");
    launch_open(ctx, b, first_col, num_cols, gl2_make(gl_canon(z[0]), gl_canon(z[1])), d_open);
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return d2h(ctx, h_out, d_open, 2 * num_cols * sizeof(gl_t));
} catch (...) { return gl_caught(); }

// The coefficient columns of the circuit's instance (glfri::PlonkInstance) over its four oracles, and where each group of the OpeningSet
// starts among them
struct FriOpenings {
    std::vector<const gl_t*> cols;          // the nopen opened at zeta, then the nnext opened at g zeta
    size_t ncs = 0, nlk = 0, nopen = 0, nnext = 0;
    size_t wires() const { return ncs; }    // where each group starts in `cols`
    size_t zs() const { return ncs + 135; }
    size_t partial_products() const { return zs() + 2; }
    size_t quotient() const { return zs() + 20; }
    size_t lookups() const { return quotient() + 16; }
    size_t zs_next() const { return nopen; }
    size_t lookups_next() const { return nopen + 2; }
};
static FriOpenings fri_openings(const gl_fri_instance& in, const gl_batch* const oracles[4]) {
    FriOpenings f;
    f.ncs = in.oracle_num_polys[0]; f.nlk = in.oracle_num_polys[2] - 20; f.nopen = in.batch_len[0]; f.nnext = in.batch_len[1];
    f.cols.reserve(f.nopen + f.nnext);
    for (size_t k = 0; k < f.nopen + f.nnext; k++) { const gl_batch* b = oracles[in.polys[2 * k]]; f.cols.push_back(b->coeffs + in.polys[2 * k + 1] * b->n); }
    return f;
}

// ---- 14. PolynomialBatch::prove_openings (fri/oracle.rs:162-219) + fri_proof (fri/prover.rs:20-216), split at every
//          transcript dependency ----
struct gl_fri {
    gl_ctx* ctx = nullptr;
    gl_fri_params params;                    // FriParams + C::Hasher: all the rounds and the queries read (no circuit behind it)
    std::vector<const gl_batch*> oracles;    // the initial trees, in the instance's oracle order
    size_t n = 0;
    uint32_t lgN = 0;
    // commit phase state
    unsigned round = 0;                      // rounds folded so far
    bool committed = false;                  // the current round's tree exists and waits for its beta
    std::unique_ptr<DevBuf> cur_vals;        // value planes [2][2^cur_lgN] of the current codeword
    std::unique_ptr<DevBuf> coef;            // coefficient planes [2][cur_n]
    size_t cur_n = 0; uint32_t cur_lgN = 0; gl_t shift = GL_MULT_GENERATOR;
    std::vector<std::unique_ptr<MerkleHolder>> trees;
    std::vector<std::unique_ptr<DevBuf>> vals;           // value planes of each committed round (query phase)
    std::vector<uint32_t> lg;
    // host sources of asynchronous uploads (alive until the object dies)
    std::vector<const gl_t*> h_cols; std::vector<gl_t> h_apow;
    std::vector<const gl_t*> h_listed_cols; std::vector<gl_t> h_listed_apow;
};
extern "C" void gl_fri_free(gl_fri* f) noexcept {
    if (!f) return;
    gl_ctx* ctx = f->ctx;
    if (ctx) (void)gl_stream_wait(ctx->stream);
    delete f;                                  // its trees and buffers go back to the context's pool first
    gl_ctx_release(ctx);
}
static gl_fri_params fri_params_of(const gl_circuit_desc& d) {
    gl_fri_params p;
    p.degree_bits = d.degree_bits; p.rate_bits = d.rate_bits; p.cap_height = d.cap_height; p.proof_of_work_bits = d.proof_of_work_bits;
    p.num_query_rounds = d.num_query_rounds; p.num_fri_rounds = d.num_fri_rounds;
    for (int r = 0; r < 8; r++) p.fri_arity_bits[r] = d.fri_arity_bits[r];
    p.hiding = d.zero_knowledge; p.hasher = d.hasher;
    return p;
}
static int fri_combine(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* const batches[4], const uint64_t zeta_in[2], const uint64_t alpha_in[2], gl_fri** out) {
    GL_TRY(check_phase_args(ctx, cir));
    GL_REQUIRE(batches && zeta_in && alpha_in && out, GL_ERR_ARG, "gl_fri_combine: null argument");
    const gl_circuit_desc& d = cir->desc;
    const size_t n = cir->n, N = n << d.rate_bits;
    const gl_fri_instance& in = cir->plonk->inst;
    for (int o = 0; o < 4; o++) GL_TRY(check_batch(cir, batches[o], in.oracle_num_polys[o], "gl_fri_combine: oracle order is constants||sigmas, wires, Z||partial products(||lookups), quotient"));
    FriOpenings op = fri_openings(in, batches);
    const size_t nopen = op.nopen, nnext = op.nnext;
    hipStream_t st = ctx->stream;
    std::unique_ptr<gl_fri, void (*)(gl_fri*)> f(new gl_fri(), gl_fri_free);
    f->ctx = ctx; ctx->retain(); f->params = fri_params_of(d); f->n = n; f->lgN = d.degree_bits + d.rate_bits;
    f->oracles.assign(batches, batches + 4);
    const gl2_t zeta = gl2_make(gl_canon(zeta_in[0]), gl_canon(zeta_in[1])), fri_alpha = gl2_make(gl_canon(alpha_in[0]), gl_canon(alpha_in[1]));
    const gl2_t gzeta = gl2_canon(gl2_scalar(zeta, gl_host_root_of_unity(d.degree_bits)));
    f->coef.reset(new DevBuf(ctx)); GL_TRY(f->coef->alloc(2 * n * sizeof(gl_t)));            // planes a, b of alpha^2 Q0 + Q1
    {
        // Both opening points in one pass (k_fri_combine_points<2> and the k_div_points_* launches, as gl_fri_combine_instance runs them):
        // the columns opened at g zeta are among those opened at zeta, so every column is read once and carries two weights.
        DevBuf d_F(ctx), d_heads(ctx), d_cols(ctx), d_wts(ctx);
        const uint32_t seg_len = (uint32_t)(n / 1024 > 32 ? n / 1024 : (n >= 32 ? 32 : n));      // at most 1024 segments
        const uint32_t nseg = (uint32_t)((n + seg_len - 1) / seg_len);
        GL_TRY(d_F.alloc(4 * n * sizeof(gl_t)));
        GL_TRY(d_heads.alloc(4 * (size_t)nseg * sizeof(gl_t)));
        GL_TRY(d_cols.alloc(nopen * sizeof(gl_t*)));
        GL_TRY(d_wts.alloc(4 * nopen * sizeof(gl_t)));
        std::vector<const gl_t*>& cols = f->h_cols;
        cols = std::move(op.cols);
        std::vector<gl_t>& wts = f->h_apow; wts.assign(4 * nopen, 0);      // [nopen][2 batches][2]; the powers of alpha depend on the proof
        { gl2_t x = gl2_make(1, 0); for (size_t j = 0; j < nopen; j++) { wts[4 * j] = x.a; wts[4 * j + 1] = x.b; x = gl2_canon(gl2_mul(x, fri_alpha)); } }
        gl2_t shift = gl2_make(1, 0);     // alpha^(#polys of batch 1) (reducing.rs:103-106)
        {
            gl2_t x = gl2_make(1, 0);
            for (size_t k = 0; k < nnext; k++) {      // polynomial k of batch 1 is column j of batch 0: the two Zs, then the lookup polynomials
                const size_t j = k < 2 ? op.zs() + k : op.lookups() + (k - 2);
                GL_REQUIRE(cols[j] == cols[nopen + k], GL_ERR_INTERNAL, "gl_fri_combine: a polynomial opened at g zeta is not where it is opened at zeta");
                wts[4 * j + 2] = x.a; wts[4 * j + 3] = x.b;
                x = gl2_canon(gl2_mul(x, fri_alpha));
            }
            shift = x;
        }
        GlFriPoints pt = {};
        pt.z[0][0] = zeta.a; pt.z[0][1] = zeta.b; pt.scale[0][0] = shift.a; pt.scale[0][1] = shift.b;      // batch 0: all polynomials at zeta
        pt.z[1][0] = gzeta.a; pt.z[1][1] = gzeta.b; pt.scale[1][0] = 1;                                    // batch 1: the Z polynomials at g * zeta
        GL_TRY(h2d_async(ctx, d_cols.p, cols.data(), nopen * sizeof(gl_t*)));
        GL_TRY(h2d_async(ctx, d_wts.p, wts.data(), wts.size() * sizeof(gl_t)));
        gl_t* F = d_F.as<gl_t>();
        gl_t* Qa = f->coef->as<gl_t>(); gl_t* Qb = Qa + n;
        const unsigned gb = (unsigned)((n + 63) / 64), sb = (nseg + 63) / 64;      // k_fri_combine_points: 64 coefficients per workgroup
        ctx->timing_begin("reduce batch + divide by linear");
        hipLaunchKernelGGL(k_fri_combine_points<2>, dim3(gb), dim3(256), 0, st, d_cols.as<const gl_t*>(), d_wts.as<gl_t>(), (uint32_t)nopen, (uint32_t)n, F);
        hipLaunchKernelGGL(k_div_points_heads, dim3(sb, 2), dim3(64), 0, st, F, (uint32_t)n, seg_len, pt, d_heads.as<gl_t>(), gl_launch_prio(128ull * sb));
        hipLaunchKernelGGL(k_div_points_carries, dim3(1, 2), dim3(1024), 0, st, d_heads.as<gl_t>(), (uint32_t)n, seg_len, pt, gl_launch_prio(2048));
        hipLaunchKernelGGL(k_div_points_apply<2>, dim3(sb), dim3(64), 0, st, F, (uint32_t)n, seg_len, pt, d_heads.as<gl_t>(), Qa, Qb);
        ctx->timing_end();
        GL_CHECK_HIP(hipGetLastError());
    }
    // final_poly.lde(rate_bits).coset_fft(7) on both planes (fri/oracle.rs:199-204)
    f->cur_vals.reset(new DevBuf(ctx)); GL_TRY(f->cur_vals->alloc(2 * N * sizeof(gl_t)));
    GL_TRY(gl_ntt_run(ctx, f->coef->as<gl_t>(), n, (uint32_t)n, f->cur_vals->as<gl_t>(), N, f->lgN, 2, false, GL_MULT_GENERATOR, 0, 1));
    f->cur_n = n; f->cur_lgN = f->lgN;
    *out = f.release();
    return GL_OK;
}
extern "C" int gl_fri_combine(gl_ctx* ctx, const gl_circuit* cir, const gl_batch* const batches[4], const uint64_t zeta_in[2], const uint64_t alpha_in[2], gl_fri** out) try {
    GL_TRY(check_phase_api(ctx, cir));
    return fri_combine(ctx, cir, batches, zeta_in, alpha_in, out);
} catch (...) { return gl_caught(); }
// fri_committed_trees, first half of one loop iteration (fri/prover.rs:76-92): Merkle tree of the current codeword
extern "C" int gl_fri_commit_round(gl_fri* f, uint64_t* h_cap_out) try {
    GL_REQUIRE(f && h_cap_out, GL_ERR_ARG, "gl_fri_commit_round: null argument");
    GL_REQUIRE(f->round < f->params.num_fri_rounds && !f->committed, GL_ERR_ARG, "gl_fri_commit_round: no round left to commit (call gl_fri_fold first)");
    gl_ctx* ctx = f->ctx;
    GL_TRY(ctx->activate());
    const uint32_t ab = f->params.fri_arity_bits[f->round], arity = 1u << ab;
    const size_t curN = size_t(1) << f->cur_lgN;
    // leaves: `arity` consecutive entries of the bit-reversed value array, flattened (fri/prover.rs:80-89)
    std::vector<uint64_t> offs(2 * arity);
    for (uint32_t k = 0; k < arity; k++)
        for (uint32_t cpt = 0; cpt < 2; cpt++) offs[2 * k + cpt] = (uint64_t)cpt * curN + (uint64_t)host_bitrev32(k, ab) * (curN >> ab);
    std::unique_ptr<MerkleHolder> tree(new MerkleHolder(ctx));
    GL_TRY(gl_merkle_build(ctx, f->cur_vals->as<gl_t>(), offs.data(), 2 * arity, f->cur_lgN - ab, f->params.cap_height, &tree->m, f->params.hasher));
    GL_TRY(d2h(ctx, h_cap_out, tree->m.level_ptr(tree->m.num_levels() - 1), (size_t(4) << f->params.cap_height) * sizeof(gl_t)));
    f->trees.push_back(std::move(tree));
    f->committed = true;
    return GL_OK;
} catch (...) { return gl_caught(); }
// second half (fri/prover.rs:94-103): fold the coefficients by beta, next codeword on the coset shift^arity
extern "C" int gl_fri_fold(gl_fri* f, const uint64_t beta_in[2]) try {
    GL_REQUIRE(f && beta_in, GL_ERR_ARG, "gl_fri_fold: null argument");
    GL_REQUIRE(f->committed, GL_ERR_ARG, "gl_fri_fold: commit the round first");
    gl_ctx* ctx = f->ctx;
    GL_TRY(ctx->activate());
    const uint32_t ab = f->params.fri_arity_bits[f->round], arity = 1u << ab;
    const gl2_t beta = gl2_make(gl_canon(beta_in[0]), gl_canon(beta_in[1]));
    const size_t next_n = f->cur_n >> ab;
    GL_REQUIRE(next_n >= 1, GL_ERR_INTERNAL, "FRI fold below one coefficient");
    std::unique_ptr<DevBuf> next(new DevBuf(ctx));
    GL_TRY(next->alloc(2 * next_n * sizeof(gl_t)));
    ctx->timing_begin("fold codewords in the commitment phase");
    hipLaunchKernelGGL(k_fri_fold, dim3((unsigned)((next_n + 255) / 256)), dim3(256), 0, ctx->stream, f->coef->as<gl_t>(), f->coef->as<gl_t>() + f->cur_n,
                       (uint32_t)next_n, arity, beta.a, beta.b, next->as<gl_t>(), next->as<gl_t>() + next_n, gl_launch_prio(next_n));
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    // the next round's state is built beside the handle and moved in at the end: a failure on the way leaves the round as it was
    const gl_t next_shift = gl_canon(gl_exp(f->shift, arity));
    const uint32_t next_lgN = f->cur_lgN - ab;
    std::unique_ptr<DevBuf> next_vals(new DevBuf(ctx));
    GL_TRY(next_vals->alloc(2 * (size_t(1) << next_lgN) * sizeof(gl_t)));
    GL_TRY(gl_ntt_run(ctx, next->as<gl_t>(), next_n, (uint32_t)next_n, next_vals->as<gl_t>(), size_t(1) << next_lgN, next_lgN, 2, false, next_shift, 0, 1));
    f->vals.reserve(f->vals.size() + 1); f->lg.reserve(f->lg.size() + 1);      // (at most 8 rounds) nothing below can fail
    f->vals.push_back(std::move(f->cur_vals)); f->lg.push_back(f->cur_lgN);
    f->cur_vals = std::move(next_vals); f->cur_lgN = next_lgN; f->shift = next_shift;
    f->coef = std::move(next);
    f->cur_n = next_n;
    f->round++; f->committed = false;
    return GL_OK;
} catch (...) { return gl_caught(); }
// final polynomial: the remaining non-zero coefficients (coeffs.truncate(len >> rate_bits), fri/prover.rs:106-111), interleaved (a, b)
extern "C" int gl_fri_final_poly(gl_fri* f, uint64_t* h_out, size_t cap_words, size_t* num_words) try {
    GL_REQUIRE(f && num_words, GL_ERR_ARG, "gl_fri_final_poly: null argument");
    GL_REQUIRE(f->round == f->params.num_fri_rounds && !f->committed, GL_ERR_ARG, "gl_fri_final_poly: reduction rounds not finished");
    *num_words = 2 * f->cur_n;
    if (!h_out) return GL_OK;
    GL_REQUIRE(cap_words >= 2 * f->cur_n, GL_ERR_ARG, "gl_fri_final_poly: output too small");
    GL_TRY(f->ctx->activate());
    std::vector<gl_t> fin(2 * f->cur_n);
    GL_TRY(d2h(f->ctx, fin.data(), f->coef->p, 2 * f->cur_n * sizeof(gl_t)));
    for (size_t i = 0; i < f->cur_n; i++) { h_out[2 * i] = fin[i]; h_out[2 * i + 1] = fin[f->cur_n + i]; }
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- fri_proof_of_work (fri/prover.rs:115-160): smallest w such that permute(state with the pending inputs and w)[7] has
//      enough leading zeros.  `sponge_state` is the Challenger's sponge, `input_buffer[0..input_len)` its pending inputs. ----
extern "C" int gl_pow_grind(gl_ctx* ctx, const uint64_t sponge_state[12], const uint64_t* input_buffer, uint32_t input_len, uint32_t min_leading_zeros, uint64_t* witness) try {
    return gl_pow_grind_h(ctx, GL_HASHER_POSEIDON, sponge_state, input_buffer, input_len, min_leading_zeros, witness);
} catch (...) { return gl_caught(); }
// fri_proof_of_work over Challenger<F, H>'s permutation, H = `hasher` (fri/prover.rs:115-160; KeccakPermutation hash/keccak.rs:64-95)
extern "C" int gl_pow_grind_h(gl_ctx* ctx, uint32_t hasher, const uint64_t sponge_state[12], const uint64_t* input_buffer, uint32_t input_len, uint32_t min_leading_zeros,
                              uint64_t* witness) try {
    GL_REQUIRE(hasher <= GL_HASHER_KECCAK, GL_ERR_ARG, "gl_pow_grind: hasher is 0 (Poseidon) or 1 (Keccak)");
    GL_REQUIRE(ctx && sponge_state && witness && (input_buffer || !input_len), GL_ERR_ARG, "gl_pow_grind: null argument");
    GL_REQUIRE(input_len < 8 && min_leading_zeros <= 40, GL_ERR_ARG, "gl_pow_grind: the witness must fit the rate (input_len < 8), at most 40 bits of work");
    GL_TRY(ctx->activate());
    hipStream_t st = ctx->stream;
    GL_TRY(ctx->ensure_dev_small(DS_BYTES));
    unsigned long long* d_res = (unsigned long long*)(ctx->dev_small + DS_POW);
    GlPowParams pw;
    // (KeccakPermutation hashes the canonical bytes of the state: canonical here, once)
    for (int i = 0; i < 12; i++) pw.state[i] = hasher == GL_HASHER_KECCAK ? gl_canon(sponge_state[i]) : sponge_state[i];
    for (uint32_t i = 0; i < input_len; i++) pw.state[i] = hasher == GL_HASHER_KECCAK ? gl_canon(input_buffer[i]) : input_buffer[i];
    pw.pos = input_len; pw.min_leading_zeros = min_leading_zeros; pw.result = d_res;
    // (measured, 16 proofs in flight: windows of 2^pow_bits, and a small grid that walks a longer window in ascending sweeps and
    // stops at the first witness -- 40 % fewer permutations -- gave the same 287 proofs/s within noise, resp. 8 % less for
    // sweeps of 2^15 lanes whose long low-occupancy launches hold up their proof; the grind is 2.7 % of a proof's instructions)
    // expected 2^pow_bits candidates: scan ascending windows of 2 * 2^pow_bits (86 % hit rate each) so that little work
    // is wasted; the window's atomicMin keeps the result the global minimum
    // (a window is at most 2^30 candidates: the grid dimension is 32 bits)
    // With several proofs in flight the extra round trips of a smaller window are hidden and the candidates hashed beyond the
    // witness are what costs: windows of 2^pow_bits (104 k candidates expected in 1.6 launches instead of 152 k in 1.2; measured
    // with 16 in flight over alternating 1920-proof runs: 294.5 / 296.6 / 296.0 / 294.9 proofs/s for windows of 2, 1, 1/2, 1/4 x 2^bits).
    static const int pow_window_env = [] { const char* e = getenv("GL_POW_WINDOW_LOG"); return e ? atoi(e) : 99; }();      // tuning knob: window = 2^(bits + this)
    const int wlog = pow_window_env != 99 ? pow_window_env : (gl_proofs_in_flight.load(std::memory_order_relaxed) > 2 ? 0 : 1);
    const int wbits = (int)min_leading_zeros + wlog < 8 ? 8 : (int)min_leading_zeros + wlog;
    const uint64_t batch = wbits >= 30 ? (uint64_t(1) << 30) : (uint64_t(1) << wbits);
    unsigned long long res = ~0ull;
    ctx->timing_begin("find proof-of-work witness");
    for (uint64_t base = 0; base < GL_P; base += batch) {
        GL_CHECK_HIP(hipMemsetAsync(d_res, 0xFF, sizeof(unsigned long long), st));
        pw.base = base; pw.count = (GL_P - base < batch) ? GL_P - base : batch; pw.prio = gl_launch_prio(pw.count);
        if (hasher == GL_HASHER_KECCAK) hipLaunchKernelGGL(k_kck_pow_grind, dim3((unsigned)((pw.count + 255) / 256)), dim3(256), 0, st, pw);
        else hipLaunchKernelGGL(k_pow_grind, dim3((unsigned)((pw.count + 255) / 256)), dim3(256), 0, st, pw);
        GL_CHECK_HIP(hipGetLastError());
        GL_TRY(d2h(ctx, &res, d_res, sizeof res));
        if (res != ~0ull) break;
    }
    ctx->timing_end();
    GL_REQUIRE(res != ~0ull, GL_ERR_INTERNAL, "Proof of work failed. This is highly unlikely!");
    *witness = (uint64_t)res;
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- fri_prover_query_rounds (fri/prover.rs:162-216): the serialised FriQueryRound list
//      (util/serialization/mod.rs:1477-1546: per query 4 x (leaf, u8 path length, siblings), then per reduction the
//      `arity` extension evaluations and the path) ----
static int fri_query_blob(gl_fri* f, const uint32_t* x_index, uint32_t nq, std::vector<uint8_t>& o) {
    gl_ctx* ctx = f->ctx;
    const gl_fri_params& d = f->params;
    const size_t no = f->oracles.size();
    hipStream_t st = ctx->stream;
    const uint32_t lgN = f->lgN;
    const size_t N = size_t(1) << lgN;
    GL_REQUIRE(f->round == d.num_fri_rounds && !f->committed, GL_ERR_ARG, "gl_fri_query: reduction rounds not finished");
    for (uint32_t q = 0; q < nq; q++) GL_REQUIRE(x_index[q] < N, GL_ERR_ARG, "gl_fri_query: query index out of range");
    // staging layout (u64 words): per oracle: rows [nq][ncols], paths [nq][levels][4]; per FRI round: leaves [nq][arity][2], paths
    struct Piece { size_t off, words; };
    std::vector<Piece> row_piece(no), path_piece(no), fleaf_piece(d.num_fri_rounds), fpath_piece(d.num_fri_rounds);
    size_t total = 0;
    const uint32_t init_levels = lgN - d.cap_height;
    for (size_t o2 = 0; o2 < no; o2++) {
        row_piece[o2] = {total, nq * f->oracles[o2]->leaf_len()}; total += row_piece[o2].words;
        path_piece[o2] = {total, (size_t)nq * init_levels * 4}; total += path_piece[o2].words;
    }
    for (unsigned r = 0; r < d.num_fri_rounds; r++) {
        const uint32_t ab = d.fri_arity_bits[r], lv = f->lg[r] - ab - d.cap_height;
        fleaf_piece[r] = {total, (size_t)nq * (2u << ab)}; total += fleaf_piece[r].words;
        fpath_piece[r] = {total, (size_t)nq * lv * 4}; total += fpath_piece[r].words;
    }
    // one upload: the piece table of k_gather_pieces, then the index lists [2 + rounds][nq]: Merkle leaf indices, natural LDE rows
    // (= bitrev(leaf)), and per FRI round the leaf index in that round's tree
    const size_t max_pieces = 2 * (no + d.num_fri_rounds), idx_words = (size_t)nq * (2 + d.num_fri_rounds);
    GL_REQUIRE(max_pieces <= GLG_MAX_PIECES, GL_ERR_INTERNAL, "gl_fri_query: more pieces than the gather table holds");
    static_assert(sizeof(GlGatherPiece) == 64, "the table is laid out in 64-byte entries ahead of the indices");
    std::vector<uint64_t> up_host(max_pieces * (sizeof(GlGatherPiece) / 8) + (idx_words + 1) / 2);
    GlGatherPiece* pieces = reinterpret_cast<GlGatherPiece*>(up_host.data());
    uint32_t* idx_host = reinterpret_cast<uint32_t*>(pieces + max_pieces);
    for (uint32_t q = 0; q < nq; q++) { idx_host[q] = x_index[q]; idx_host[nq + q] = host_bitrev32(x_index[q], lgN); }
    {
        std::vector<uint32_t> xi(x_index, x_index + nq);
        for (unsigned r = 0; r < d.num_fri_rounds; r++) for (uint32_t q = 0; q < nq; q++) { xi[q] >>= d.fri_arity_bits[r]; idx_host[(size_t)(2 + r) * nq + q] = xi[q]; }
    }
    uint32_t npieces = 0, nblocks = 0;
    auto add_piece = [&](uint32_t kind, const gl_t* src, const gl_t* src2, const uint64_t* level_off, uint64_t stride, uint32_t a, uint32_t b2, size_t count,
                         size_t idx_off, size_t out_off) {
        if (!count) return;
        pieces[npieces++] = GlGatherPiece{src, src2, level_off, stride, (uint64_t)out_off, kind, a, b2, (uint32_t)count, (uint32_t)idx_off, 0};
        nblocks += (uint32_t)((count + 255) / 256);
    };
    for (size_t o2 = 0; o2 < no; o2++) {
        const gl_batch* b = f->oracles[o2];
        const uint64_t* d_lo = nullptr;
        GL_TRY(ctx->get_offsets_table(b->tree.level_off.data(), b->tree.level_off.size(), &d_lo));
        // the whole leaf: with blinding the salt follows the values (query rounds open salted leaves)
        add_piece(GLG_ROWS, b->lde, nullptr, nullptr, (uint64_t)N, (uint32_t)b->leaf_len(), 0, (size_t)nq * b->leaf_len(), nq, row_piece[o2].off);
        add_piece(GLG_PATHS, b->tree.digests, nullptr, d_lo, 0, init_levels, 0, (size_t)nq * init_levels * 4, 0, path_piece[o2].off);
    }
    for (unsigned r = 0; r < d.num_fri_rounds; r++) {
        const uint32_t ab = d.fri_arity_bits[r], lv = f->lg[r] - ab - d.cap_height;
        const GlMerkle& t = f->trees[r]->m;
        const uint64_t* d_lo = nullptr;
        GL_TRY(ctx->get_offsets_table(t.level_off.data(), t.level_off.size(), &d_lo));
        const gl_t* va = f->vals[r]->as<gl_t>(); const gl_t* vb = va + (size_t(1) << f->lg[r]);
        add_piece(GLG_FRI_LEAVES, va, vb, nullptr, 0, ab, f->lg[r], (size_t)nq << ab, (size_t)(2 + r) * nq, fleaf_piece[r].off);
        add_piece(GLG_PATHS, t.digests, nullptr, d_lo, 0, lv, 0, (size_t)nq * lv * 4, (size_t)(2 + r) * nq, fpath_piece[r].off);
    }
    DevBuf d_stage(ctx), d_up(ctx);
    GL_TRY(d_stage.alloc((total + 8) * sizeof(gl_t)));
    GL_TRY(d_up.alloc(up_host.size() * sizeof(uint64_t)));
    GL_TRY(h2d_async(ctx, d_up.p, up_host.data(), up_host.size() * sizeof(uint64_t)));
    gl_t* stage = d_stage.as<gl_t>();
    ctx->timing_begin("FRI query gathers");
    if (nblocks)
        hipLaunchKernelGGL(k_gather_pieces, dim3(nblocks), dim3(256), 0, st, d_up.as<GlGatherPiece>(), npieces,
                           reinterpret_cast<const uint32_t*>(d_up.as<GlGatherPiece>() + max_pieces), stage, gl_launch_prio(256ull * nblocks));
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    std::vector<gl_t> host_stage(total + 8);
    GL_TRY(d2h(ctx, host_stage.data(), stage, total * sizeof(gl_t)));      // also orders the idx_host upload before it dies
    for (uint32_t q = 0; q < nq; q++) {
        for (size_t oi = 0; oi < no; oi++) {
            const size_t nc = f->oracles[oi]->leaf_len();
            put_words(o, host_stage.data() + row_piece[oi].off + (size_t)q * nc, nc);
            o.push_back((uint8_t)init_levels);
            put_hashes(o, d.hasher, host_stage.data() + path_piece[oi].off + (size_t)q * init_levels * 4, init_levels);
        }
        for (unsigned r = 0; r < d.num_fri_rounds; r++) {
            const uint32_t ab = d.fri_arity_bits[r], lv = f->lg[r] - ab - d.cap_height;
            put_words(o, host_stage.data() + fleaf_piece[r].off + (size_t)q * (2u << ab), 2u << ab);
            o.push_back((uint8_t)lv);
            put_hashes(o, d.hasher, host_stage.data() + fpath_piece[r].off + (size_t)q * lv * 4, lv);
        }
    }
    return GL_OK;
}
extern "C" int gl_fri_query(gl_fri* f, const uint32_t* x_index, uint32_t num_queries, uint8_t* h_blob, size_t cap_bytes, size_t* num_bytes) try {
    GL_REQUIRE(f && x_index && num_bytes, GL_ERR_ARG, "gl_fri_query: null argument");
    GL_REQUIRE(num_queries >= 1 && num_queries <= 256, GL_ERR_ARG, "gl_fri_query: 1..256 queries");
    GL_TRY(f->ctx->activate());
    std::vector<uint8_t> blob;
    GL_TRY(fri_query_blob(f, x_index, num_queries, blob));
    *num_bytes = blob.size();
    if (!h_blob) return GL_OK;
    GL_REQUIRE(cap_bytes >= blob.size(), GL_ERR_ARG, "gl_fri_query: output too small");
    memcpy(h_blob, blob.data(), blob.size());
    return GL_OK;
} catch (...) { return gl_caught(); }

// ---- PolynomialBatch::prove_openings for any FriInstanceInfo (fri/oracle.rs:162-219, fri/structure.rs) ----
static_assert(GLF_MAX_POINTS == GL_MAX_FRI_BATCHES, "the kernels' point table holds one entry per batch");
static int check_instance_batches(gl_ctx* ctx, const gl_fri_params& p, const gl_fri_instance& in, const gl_batch* const* batches) {
    GL_REQUIRE(batches, GL_ERR_ARG, "FRI openings: null batch list");
    for (uint32_t o = 0; o < in.num_oracles; o++) {
        const gl_batch* b = batches[o];
        GL_REQUIRE(b && b->ctx && b->ctx->device == ctx->device, GL_ERR_ARG, "FRI openings: a null batch, or one on another device");
        GL_REQUIRE(b->n == (size_t(1) << p.degree_bits) && b->rate_bits == p.rate_bits && b->cap_height == p.cap_height && b->ncols == in.oracle_num_polys[o],
                   GL_ERR_ARG, "FRI openings: a batch whose degree, rate_bits, cap_height or column count differs from params / instance");
        GL_REQUIRE(b->hasher == p.hasher, GL_ERR_ARG, "a batch committed under another hasher than the params'");
        GL_REQUIRE(b->salt == glfri::salt_of(p, in, o), GL_ERR_ARG, "FRI openings: a batch is salted where the instance is not blinded (or the reverse)");
    }
    return GL_OK;
}
// `per_batch`: the sequence gl_fri_combine ran before it used the one-pass kernels, one batch after the other (k_fri_combine + the three division launches, every listed
// column read where it is listed) -- what tools/openings_rate.py measures the one-pass kernels against
static int fri_combine_instance(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches, const uint64_t alpha_in[2], gl_fri** out,
                                bool per_batch = false) {
    GL_REQUIRE(ctx && alpha_in && out, GL_ERR_ARG, "gl_fri_combine_instance: null argument");
    GL_TRY(glfri::check(params, instance, true));
    const gl_fri_params& p = *params; const gl_fri_instance& in = *instance;
    GL_TRY(check_instance_batches(ctx, p, in, batches));
    GL_TRY(ctx->activate());
    const size_t n = size_t(1) << p.degree_bits, N = n << p.rate_bits;
    const uint32_t B = in.num_batches;
    hipStream_t st = ctx->stream;
    std::unique_ptr<gl_fri, void (*)(gl_fri*)> f(new gl_fri(), gl_fri_free);
    f->ctx = ctx; ctx->retain(); f->params = p; f->n = n; f->lgN = p.degree_bits + p.rate_bits;
    f->oracles.assign(batches, batches + in.num_oracles);
    const gl2_t alpha = gl2_make(gl_canon(alpha_in[0]), gl_canon(alpha_in[1]));
    // the distinct columns in order of first appearance, and per column and batch the sum of the powers of alpha it takes there
    // (reduce_polys_base, reducing.rs:83-95: polynomial j of a batch takes alpha^j)
    size_t first_col[GL_MAX_FRI_ORACLES + 1] = {0};
    for (uint32_t o = 0; o < in.num_oracles; o++) first_col[o + 1] = first_col[o] + in.oracle_num_polys[o];
    std::vector<int32_t> slot(first_col[in.num_oracles], -1);
    std::vector<const gl_t*>& cols = f->h_cols;
    std::vector<gl_t>& wts = f->h_apow;
    std::vector<const gl_t*>& listed_cols = f->h_listed_cols;      // per_batch: the columns as listed, and alpha^j of each
    std::vector<gl_t>& listed_apow = f->h_listed_apow;
    GlFriPoints pt;
    gl2_t alpha_len[GL_MAX_FRI_BATCHES];                    // alpha^(len of batch b)
    for (uint32_t b = 0, k = 0; b < B; b++) {
        gl2_t x = gl2_make(1, 0);
        for (uint32_t j = 0; j < in.batch_len[b]; j++, k++) {
            const uint32_t o = in.polys[2 * k], c = in.polys[2 * k + 1];
            int32_t& sl = slot[first_col[o] + c];
            if (sl < 0) { sl = (int32_t)cols.size(); cols.push_back(batches[o]->coeffs + (size_t)c * n); wts.resize(wts.size() + 2 * B, 0); }
            gl_t* w = &wts[(size_t)sl * 2 * B + 2 * b];
            w[0] = gl_canon(gl_add(w[0], x.a)); w[1] = gl_canon(gl_add(w[1], x.b));
            if (per_batch) { listed_cols.push_back(batches[o]->coeffs + (size_t)c * n); listed_apow.push_back(x.a); listed_apow.push_back(x.b); }
            x = gl2_canon(gl2_mul(x, alpha));
        }
        alpha_len[b] = x;
    }
    {   // shift_poly (reducing.rs:103-106): quotient b is multiplied by alpha^len of every later batch
        gl2_t s = gl2_make(1, 0);
        for (uint32_t b = GL_MAX_FRI_BATCHES; b-- > 0;) {
            const gl2_t z = b < B ? glfri::point_of(in, b) : gl2_make(0, 0);
            pt.z[b][0] = z.a; pt.z[b][1] = z.b;
            pt.scale[b][0] = b < B ? s.a : 0; pt.scale[b][1] = b < B ? s.b : 0;
            if (b < B) s = gl2_canon(gl2_mul(s, alpha_len[b]));
        }
    }
    const size_t ncols = cols.size();
    f->coef.reset(new DevBuf(ctx)); GL_TRY(f->coef->alloc(2 * n * sizeof(gl_t)));
    {
        DevBuf d_F(ctx), d_heads(ctx), d_cols(ctx), d_wts(ctx);
        const uint32_t seg_len = (uint32_t)(n / 1024 > 32 ? n / 1024 : (n >= 32 ? 32 : n));      // at most 1024 segments
        const uint32_t nseg = (uint32_t)((n + seg_len - 1) / seg_len);
        GL_TRY(d_F.alloc(2 * (size_t)B * n * sizeof(gl_t)));
        GL_TRY(d_heads.alloc(2 * (size_t)B * nseg * sizeof(gl_t)));
        GL_TRY(d_cols.alloc(ncols * sizeof(gl_t*)));
        GL_TRY(d_wts.alloc(wts.size() * sizeof(gl_t)));
        GL_TRY(h2d_async(ctx, d_cols.p, cols.data(), ncols * sizeof(gl_t*)));
        GL_TRY(h2d_async(ctx, d_wts.p, wts.data(), wts.size() * sizeof(gl_t)));
        gl_t* F = d_F.as<gl_t>();
        gl_t* Qa = f->coef->as<gl_t>(); gl_t* Qb = Qa + n;
        const unsigned gb = (unsigned)((n + 63) / 64), sb = (nseg + 63) / 64;
        if (per_batch) {
            DevBuf d_lcols(ctx), d_lapow(ctx);
            GL_TRY(d_lcols.alloc(listed_cols.size() * sizeof(gl_t*)));
            GL_TRY(d_lapow.alloc(listed_apow.size() * sizeof(gl_t)));
            GL_TRY(h2d_async(ctx, d_lcols.p, listed_cols.data(), listed_cols.size() * sizeof(gl_t*)));
            GL_TRY(h2d_async(ctx, d_lapow.p, listed_apow.data(), listed_apow.size() * sizeof(gl_t)));
            gl_t* Fa = F; gl_t* Fb = F + n;
            ctx->timing_begin("reduce batch + divide by linear, batch after batch");
            for (uint32_t b = 0, k = 0; b < B; k += in.batch_len[b], b++) {
                hipLaunchKernelGGL(k_fri_combine, dim3(gb), dim3(256), 0, st, d_lcols.as<const gl_t*>() + k, d_lapow.as<gl_t>() + 2 * k, in.batch_len[b], (uint32_t)n, Fa, Fb);
                hipLaunchKernelGGL(k_div_linear_heads, dim3(sb), dim3(64), 0, st, Fa, Fb, (uint32_t)n, seg_len, pt.z[b][0], pt.z[b][1], d_heads.as<gl_t>());
                hipLaunchKernelGGL(k_div_linear_carries, dim3(1), dim3(1024), 0, st, d_heads.as<gl_t>(), (uint32_t)n, seg_len, pt.z[b][0], pt.z[b][1]);
                hipLaunchKernelGGL(k_div_linear_apply, dim3(sb), dim3(64), 0, st, Fa, Fb, (uint32_t)n, seg_len, pt.z[b][0], pt.z[b][1], d_heads.as<gl_t>(), pt.scale[b][0],
                                   pt.scale[b][1], Qa, Qb, b ? 1 : 0);
            }
            ctx->timing_end();
            GL_CHECK_HIP(hipGetLastError());
        } else {
        ctx->timing_begin("reduce batches + divide by linear");
#define GLF_LAUNCH(NB)                                                                                                                               \
    case NB:                                                                                                                                         \
        hipLaunchKernelGGL(k_fri_combine_points<NB>, dim3(gb), dim3(256), 0, st, d_cols.as<const gl_t*>(), d_wts.as<gl_t>(), (uint32_t)ncols, (uint32_t)n, F); \
        hipLaunchKernelGGL(k_div_points_heads, dim3(sb, NB), dim3(64), 0, st, F, (uint32_t)n, seg_len, pt, d_heads.as<gl_t>(), gl_launch_prio(64ull * NB * sb)); \
        hipLaunchKernelGGL(k_div_points_carries, dim3(1, NB), dim3(1024), 0, st, d_heads.as<gl_t>(), (uint32_t)n, seg_len, pt, gl_launch_prio(1024ull * NB)); \
        hipLaunchKernelGGL(k_div_points_apply<NB>, dim3(sb), dim3(64), 0, st, F, (uint32_t)n, seg_len, pt, d_heads.as<gl_t>(), Qa, Qb);               \
        break;
        switch (B) { GLF_LAUNCH(1) GLF_LAUNCH(2) GLF_LAUNCH(3) GLF_LAUNCH(4) }
#undef GLF_LAUNCH
        ctx->timing_end();
        GL_CHECK_HIP(hipGetLastError());
        }
    }
    // final_poly.lde(rate_bits).coset_fft(7) on both planes (fri/oracle.rs:199-204)
    f->cur_vals.reset(new DevBuf(ctx)); GL_TRY(f->cur_vals->alloc(2 * N * sizeof(gl_t)));
    GL_TRY(gl_ntt_run(ctx, f->coef->as<gl_t>(), n, (uint32_t)n, f->cur_vals->as<gl_t>(), N, f->lgN, 2, false, GL_MULT_GENERATOR, 0, 1));
    f->cur_n = n; f->cur_lgN = f->lgN;
    *out = f.release();
    return GL_OK;
}
extern "C" int gl_fri_combine_instance(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches,
                                       const uint64_t alpha[2], gl_fri** out) try {
    return fri_combine_instance(ctx, params, instance, batches, alpha, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_fri_combine_instance_per_batch(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches,
                                                 const uint64_t alpha[2], gl_fri** out) try {
    return fri_combine_instance(ctx, params, instance, batches, alpha, out, true);
} catch (...) { return gl_caught(); }
// fri_proof (fri/prover.rs:20-66) behind it, on the caller's Challenger; the FriProof in write_fri_proof order (util/serialization/mod.rs:1568-1582)
extern "C" int gl_prove_openings(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches,
                                 gl_challenger* challenger, uint8_t* h_out, size_t cap_bytes, size_t* num_bytes) try {
    GL_REQUIRE(ctx && challenger && num_bytes, GL_ERR_ARG, "gl_prove_openings: null argument");
    GL_TRY(glfri::check(params, instance, true));
    const gl_fri_params& p = *params; const gl_fri_instance& in = *instance;
    GL_TRY(check_instance_batches(ctx, p, in, batches));
    GL_REQUIRE(challenger->ch.hasher == p.hasher, GL_ERR_ARG, "gl_prove_openings: the challenger runs under another hasher than the params'");
    const uint32_t lgN = p.degree_bits + p.rate_bits, ncap = 4u << p.cap_height;
    const size_t N = size_t(1) << lgN, size = glfri::proof_bytes(p, in);
    *num_bytes = size;
    if (!h_out) return GL_OK;                          // the size alone: nothing ran, the challenger is where it was
    GL_REQUIRE(cap_bytes >= size, GL_ERR_ARG, "gl_prove_openings: output too small");
    HostChallenger& ch = challenger->ch;
    const gl2_t alpha = ch.challenge_ext();
    const gl_t alpha_w[2] = {alpha.a, alpha.b};
    gl_fri* fri_raw = nullptr;
    GL_TRY(fri_combine_instance(ctx, params, instance, batches, alpha_w, &fri_raw));
    std::unique_ptr<gl_fri, void (*)(gl_fri*)> fri(fri_raw, gl_fri_free);
    std::vector<uint8_t> o;
    o.reserve(size);
    std::vector<gl_t> cap(ncap);
    for (unsigned r = 0; r < p.num_fri_rounds; r++) {
        GL_TRY(gl_fri_commit_round(fri.get(), cap.data()));
        put_hashes(o, p.hasher, cap.data(), ncap / 4);
        ch.observe_hashes(p.hasher, cap.data(), ncap / 4);
        const gl2_t beta = ch.challenge_ext();
        const gl_t beta_w[2] = {beta.a, beta.b};
        GL_TRY(gl_fri_fold(fri.get(), beta_w));
    }
    size_t fin_words = 0;
    GL_TRY(gl_fri_final_poly(fri.get(), nullptr, 0, &fin_words));
    std::vector<gl_t> fin_il(fin_words);
    GL_TRY(gl_fri_final_poly(fri.get(), fin_il.data(), fin_il.size(), &fin_words));
    ch.observe_many(fin_il.data(), fin_il.size());
    gl_t pow_witness = 0;
    GL_TRY(gl_pow_grind_h(ctx, p.hasher, ch.state, ch.in, (uint32_t)ch.nin, p.proof_of_work_bits, &pow_witness));
    ch.observe(pow_witness);
    const gl_t pow_response = ch.challenge();
    GL_REQUIRE(pow_response == 0 || (uint32_t)__builtin_clzll(pow_response) >= p.proof_of_work_bits, GL_ERR_INTERNAL, "PoW response mismatch");
    std::vector<uint32_t> x_index(p.num_query_rounds);
    for (auto& x : x_index) x = (uint32_t)(ch.challenge() % (uint64_t)N);
    GL_TRY(fri_query_blob(fri.get(), x_index.data(), p.num_query_rounds, o));
    put_words(o, fin_il.data(), fin_il.size());
    put_u64(o, pow_witness);
    GL_REQUIRE(o.size() == size, GL_ERR_INTERNAL, "gl_prove_openings: the proof is not as long as its parameters say");
    memcpy(h_out, o.data(), size);
    return GL_OK;
} catch (...) { return gl_caught(); }

// ======================================================================================================================
// prove(): the driver (plonk/prover.rs:102-329) -- the phases above plus the transcript
// ======================================================================================================================
// `d_wires` is the witness [135][n] in HBM; `wit_owner`, if given, owns it and is released once the last kernel that reads it is queued
// `seed`: the salt key of a zero-knowledge circuit (null = OS entropy); unused without zero knowledge
static int prove_impl(gl_ctx* ctx, const gl_circuit* cir, const gl_t* d_wires, DevBuf* wit_owner, const uint64_t* h_pis, size_t npis, const uint64_t* h_pi_hash, gl_proof** out,
                      const uint8_t* seed = nullptr) {
    GL_REQUIRE(ctx && cir && d_wires && h_pis && out, GL_ERR_ARG, "gl_prove: null argument");
    // circuit data is read-only while proving: any context (stream) of the same device may prove against it
    GL_REQUIRE(cir->ctx->device == ctx->device, GL_ERR_ARG, "gl_prove: circuit lives on another device");
    const gl_circuit_desc& d = cir->desc;
    GL_REQUIRE(npis == d.num_public_inputs, GL_ERR_ARG, "gl_prove: wrong number of public inputs");
    GL_TRY(ctx->activate());
    struct InFlight { InFlight() { gl_proofs_in_flight.fetch_add(1, std::memory_order_relaxed); } ~InFlight() { gl_proofs_in_flight.fetch_sub(1, std::memory_order_relaxed); } } in_flight;
    const size_t n = cir->n, N = n << d.rate_bits;
    const uint32_t lgn = d.degree_bits, ncap = 4u << d.cap_height;
    hipStream_t st = ctx->stream;
    std::unique_ptr<gl_proof> proof(new gl_proof());
    std::vector<gl_t> h_apow_quot;          // sources of async uploads: alive until the function returns (after the last sync)

    // zero knowledge: wires, Z || partial products and quotient are committed with blinding = true (prover.rs:151,218,266)
    uint8_t salt_seed[32];
    const uint8_t* salt = nullptr;
    if (d.zero_knowledge) {
        if (seed) memcpy(salt_seed, seed, 32);
        else GL_TRY(gl_os_seed(salt_seed));
        salt = salt_seed;
    }

    // ---- 4. wires commitment (prover.rs:145-156) ----
    BatchHolder wires; GL_TRY(gl_batch_from_device_salted(ctx, d_wires, 135, n, d.rate_bits, d.cap_height, 1, salt, 1, &wires.b, d.hasher));
    // public_inputs_hash (prover.rs:126-127) on the host while the GPU commits
    gl_t pi_hash[4];
    if (h_pi_hash) for (int i = 0; i < 4; i++) pi_hash[i] = gl_canon(h_pi_hash[i]);      // the witness generator's sponge already produced it
    else glhost::host_hash_no_pad(h_pis, npis, pi_hash);
    // Challenger<F, C::Hasher>: circuit_digest is a C::Hasher hash, public_inputs_hash a C::InnerHasher (Poseidon) one (prover.rs:158-161)
    HostChallenger ch(d.hasher);
    ch.observe_hashes(d.hasher, cir->circuit_digest, 1);
    ch.observe_many(pi_hash, 4);
    std::vector<gl_t> cap(ncap);
    GL_TRY(gl_batch_cap(wires.b, cap.data()));
    proof->caps.insert(proof->caps.end(), cap.begin(), cap.end());
    ch.observe_hashes(d.hasher, cap.data(), ncap / 4);
    gl_t betas[2], gammas[2], alphas[2];
    for (int i = 0; i < 2; i++) betas[i] = ch.challenge();
    for (int i = 0; i < 2; i++) gammas[i] = ch.challenge();
    // lookups: four coins per challenge, [betas | gammas | 4 more] (prover.rs:166-184)
    gl_t deltas[8] = {betas[0], betas[1], gammas[0], gammas[1], 0, 0, 0, 0};
    const gl_t* lookup_deltas = d.num_lookup_polys ? deltas : nullptr;
    if (lookup_deltas) for (int i = 4; i < 8; i++) deltas[i] = ch.challenge();

    // ---- 6/7. partial products and Z (and the lookup polynomials), commitment (prover.rs:189-223) ----
    BatchHolder zs;
    GL_TRY(commit_zs(ctx, cir, d_wires, betas, gammas, lookup_deltas, &zs.b, ctx->capture_intermediates ? &proof->zs_pp : nullptr, salt));
    if (wit_owner) wit_owner->release();                                       // stream-ordered: the kernels above are already queued
    GL_TRY(gl_batch_cap(zs.b, cap.data()));
    proof->caps.insert(proof->caps.end(), cap.begin(), cap.end());
    ch.observe_hashes(d.hasher, cap.data(), ncap / 4);
    for (int i = 0; i < 2; i++) alphas[i] = ch.challenge();

    // ---- 9/10. quotient polynomials (prover.rs:229-271) ----
    BatchHolder quot;
    GL_TRY(commit_quotient(ctx, cir, wires.b, zs.b, pi_hash, betas, gammas, alphas, lookup_deltas, h_apow_quot, &quot.b, ctx->capture_intermediates ? &proof->quotient : nullptr,
                           salt));
    GL_TRY(gl_batch_cap(quot.b, cap.data()));
    proof->caps.insert(proof->caps.end(), cap.begin(), cap.end());
    ch.observe_hashes(d.hasher, cap.data(), ncap / 4);

    // ---- 11. zeta (prover.rs:273-283) ----
    const gl2_t zeta = ch.challenge_ext();
    {
        gl2_t zn = zeta;
        for (uint32_t i = 0; i < lgn; i++) zn = gl2_mul(zn, zn);
        zn = gl2_canon(zn);
        if (zn.a == 1 && zn.b == 0) return gl_fail(GL_ERR_ZETA_IN_SUBGROUP, "Opening point is in the subgroup.", __FILE__, __LINE__);
    }
    const gl2_t gzeta = gl2_canon(gl2_scalar(zeta, gl_host_root_of_unity(lgn)));

    // ---- 12. openings (proof.rs:306-344): all of them in one launch behind one sync (gl_open_at is one batch per call) ----
    const gl_batch* oracles[4] = {cir->cs_batch, wires.b, zs.b, quot.b};
    const FriOpenings op = fri_openings(cir->plonk->inst, oracles);
    GL_REQUIRE(op.nopen + op.nnext <= DS_OPEN_MAX, GL_ERR_INTERNAL, "too many openings for the staging area");
    std::vector<gl_t> opened(2 * (op.nopen + op.nnext));                       // extension values, in op.cols order
    {
        GL_TRY(ctx->ensure_dev_small(DS_BYTES));
        gl_t* d_open = ctx->dev_small + DS_OPEN;
        ctx->timing_begin("construct the opening set");
        // zeta^i and (g zeta)^i tabulated once per proof, shared by all polynomials
        DevBuf d_zpow(ctx); GL_TRY(d_zpow.alloc(4 * n * sizeof(gl_t)));
        gl_t* zp = d_zpow.as<gl_t>();
        hipLaunchKernelGGL(k_ext_powers2, dim3((unsigned)((n + 255) / 256), 2), dim3(256), 0, st, zeta.a, zeta.b, gzeta.a, gzeta.b, (uint32_t)n, zp, gl_launch_prio(2 * n));
        // the list of coefficient columns goes up as a small pointer table
        DevBuf d_open_cols(ctx); GL_TRY(d_open_cols.alloc(op.cols.size() * sizeof(gl_t*)));
        GL_TRY(h2d_async(ctx, d_open_cols.p, op.cols.data(), op.cols.size() * sizeof(gl_t*)));
        hipLaunchKernelGGL(k_eval_list_with_powers, dim3((unsigned)op.cols.size()), dim3(256), 0, st, d_open_cols.as<const gl_t*>(), (uint32_t)n,
                           (uint32_t)op.nopen, zp, zp + n, zp + 2 * n, zp + 3 * n, d_open);
        ctx->timing_end();
        GL_CHECK_HIP(hipGetLastError());
        GL_TRY(d2h(ctx, opened.data(), d_open, opened.size() * sizeof(gl_t)));
    }
    ch.observe_many(opened.data(), opened.size());

    // ---- 14. prove_openings (fri/oracle.rs:162-219), fri_proof (fri/prover.rs:20-66) ----
    const gl2_t fri_alpha = ch.challenge_ext();
    const gl_t zeta_w[2] = {zeta.a, zeta.b}, fri_alpha_w[2] = {fri_alpha.a, fri_alpha.b};
    gl_fri* fri_raw = nullptr;
    GL_TRY(fri_combine(ctx, cir, oracles, zeta_w, fri_alpha_w, &fri_raw));
    std::unique_ptr<gl_fri, void (*)(gl_fri*)> fri(fri_raw, gl_fri_free);
    std::vector<gl_t> fri_caps, fri_betas;
    for (unsigned r = 0; r < d.num_fri_rounds; r++) {
        GL_TRY(gl_fri_commit_round(fri.get(), cap.data()));
        fri_caps.insert(fri_caps.end(), cap.begin(), cap.end());
        ch.observe_hashes(d.hasher, cap.data(), ncap / 4);
        const gl2_t beta = ch.challenge_ext();
        const gl_t beta_w[2] = {beta.a, beta.b};
        fri_betas.insert(fri_betas.end(), beta_w, beta_w + 2);
        GL_TRY(gl_fri_fold(fri.get(), beta_w));
    }
    size_t fin_words = 0;
    GL_TRY(gl_fri_final_poly(fri.get(), nullptr, 0, &fin_words));
    std::vector<gl_t> fin_il(fin_words);
    GL_TRY(gl_fri_final_poly(fri.get(), fin_il.data(), fin_il.size(), &fin_words));
    ch.observe_many(fin_il.data(), fin_il.size());
    gl_t pow_witness = 0;
    GL_TRY(gl_pow_grind_h(ctx, d.hasher, ch.state, ch.in, (uint32_t)ch.nin, d.proof_of_work_bits, &pow_witness));
    ch.observe(pow_witness);
    const gl_t pow_response = ch.challenge();
    GL_REQUIRE(pow_response == 0 || (uint32_t)__builtin_clzll(pow_response) >= d.proof_of_work_bits, GL_ERR_INTERNAL, "PoW response mismatch");
    const uint32_t nq = d.num_query_rounds;
    std::vector<uint32_t> x_index(nq);
    for (uint32_t q = 0; q < nq; q++) { x_index[q] = (uint32_t)(ch.challenge() % (uint64_t)N); proof->query_indices.push_back(x_index[q]); }
    std::vector<uint8_t> query_blob;
    query_blob.reserve(200000);
    GL_TRY(fri_query_blob(fri.get(), x_index.data(), nq, query_blob));

    // ---- 15. assemble ProofWithPublicInputs bytes (util/serialization/mod.rs:1939-1981) ----
    std::vector<uint8_t>& o = proof->bytes;
    o.reserve(query_blob.size() + 8 * (npis + 2 * op.nopen + fin_words + 4 * ncap) + 4096);
    put_hashes(o, d.hasher, proof->caps.data(), proof->caps.size() / 4);           // wires_cap, zs_pp_cap, quotient_cap
    // OpeningSet (:1409-1423): constants, sigmas, wires, zs, zs_next, lookup_zs, lookup_zs_next, partial products, quotient
    const gl_t* z = opened.data();
    put_words(o, z, 2 * op.ncs);
    put_words(o, z + 2 * op.wires(), 2 * 135);
    put_words(o, z + 2 * op.zs(), 2 * 2);
    put_words(o, z + 2 * op.zs_next(), 2 * 2);
    put_words(o, z + 2 * op.lookups(), 2 * op.nlk);
    put_words(o, z + 2 * op.lookups_next(), 2 * op.nlk);
    put_words(o, z + 2 * op.partial_products(), 2 * 18);
    put_words(o, z + 2 * op.quotient(), 2 * 16);
    put_hashes(o, d.hasher, fri_caps.data(), fri_caps.size() / 4);
    o.insert(o.end(), query_blob.begin(), query_blob.end());
    put_words(o, fin_il.data(), fin_il.size());
    put_u64(o, pow_witness);
    put_u64(o, npis);
    put_words(o, h_pis, npis);

    std::vector<gl_t>& cv = proof->challenges;
    for (int i = 0; i < 2; i++) cv.push_back(betas[i]);
    for (int i = 0; i < 2; i++) cv.push_back(gammas[i]);
    for (int i = 0; i < 2; i++) cv.push_back(alphas[i]);
    cv.push_back(zeta.a); cv.push_back(zeta.b); cv.push_back(fri_alpha.a); cv.push_back(fri_alpha.b); cv.push_back(pow_witness);
    for (int i = 0; i < 4; i++) cv.push_back(pi_hash[i]);
    cv.insert(cv.end(), fri_betas.begin(), fri_betas.end());
    GL_CHECK_HIP(gl_stream_wait(st));
    *out = proof.release();
    return GL_OK;
}
// host witness -> HBM, then prove(): gl_prove (one [135][n] matrix) and gl_prove_columns (135 vectors).  The caller's memory has been
// read when h2d_witness returns; prove_impl releases the device copy.
static int prove_host_witness(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* const* cols, const uint64_t* flat, const uint64_t* h_pis, size_t npis, gl_proof** out) {
    GL_TRY(ctx->activate());
    DevBuf d_wit(ctx); GL_TRY(d_wit.alloc(135 * cir->n * sizeof(gl_t)));
    ctx->timing_begin("H2D witness");
    GL_TRY(h2d_witness(ctx, d_wit.as<gl_t>(), 135, cir->n, cols, flat));
    ctx->timing_end();
    return prove_impl(ctx, cir, d_wit.as<gl_t>(), &d_wit, h_pis, npis, nullptr, out);
}
extern "C" int gl_prove(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* h_wires, const uint64_t* h_pis, size_t npis, gl_proof** out) try {
    GL_REQUIRE(ctx && cir && h_wires && out, GL_ERR_ARG, "gl_prove: null argument");
    return prove_host_witness(ctx, cir, nullptr, h_wires, h_pis, npis, out);
} catch (...) { return gl_caught(); }
// the witness as the reference holds it: one host vector per wire (MatrixWitness.wire_values: Vec<Vec<F>>, iop/witness.rs:256-258)
extern "C" int gl_prove_columns(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* const* h_wire_columns, const uint64_t* h_pis, size_t npis, gl_proof** out) try {
    GL_REQUIRE(ctx && cir && h_wire_columns && out, GL_ERR_ARG, "gl_prove_columns: null argument");
    for (size_t c = 0; c < 135; c++) GL_REQUIRE(h_wire_columns[c], GL_ERR_ARG, "gl_prove_columns: null column");
    return prove_host_witness(ctx, cir, h_wire_columns, nullptr, h_pis, npis, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_prove_device(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t* h_pis, size_t npis, gl_proof** out) try {
    return prove_impl(ctx, cir, d_wires, nullptr, h_pis, npis, nullptr, out);
} catch (...) { return gl_caught(); }
extern "C" int gl_prove_device_seeded(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t* h_pis, size_t npis, const uint8_t seed[32],
                                      gl_proof** out) try {
    return prove_impl(ctx, cir, d_wires, nullptr, h_pis, npis, nullptr, out, seed);
} catch (...) { return gl_caught(); }
extern "C" int gl_witness_blind(gl_ctx* ctx, const gl_circuit* cir, uint64_t* d_wires, const uint8_t seed[32]) try {
    GL_REQUIRE(ctx && cir && d_wires, GL_ERR_ARG, "gl_witness_blind: null argument");
    GL_REQUIRE(cir->ctx->device == ctx->device, GL_ERR_ARG, "gl_witness_blind: circuit lives on another device");
    const gl_circuit_desc& d = cir->desc;
    GL_REQUIRE(d.zero_knowledge && d.num_gate_rows, GL_ERR_ARG, "gl_witness_blind: needs a zero-knowledge circuit with num_gate_rows set");
    GL_TRY(ctx->activate());
    const glhost::BlindingCounts b = glhost::blinding_counts(d.num_gate_rows, true, d.rate_bits, d.cap_height, d.num_query_rounds);
    uint8_t os[32];
    if (!seed) { GL_TRY(gl_os_seed(os)); seed = os; }
    return gl_launch_witness_blind(ctx, seed, d_wires, (uint32_t)cir->n, d.num_gate_rows, b.regular, b.pairs);
} catch (...) { return gl_caught(); }
extern "C" int gl_prove_device_hashed(gl_ctx* ctx, const gl_circuit* cir, const uint64_t* d_wires, const uint64_t* h_pis, size_t npis,
                                      const uint64_t public_inputs_hash[4], gl_proof** out) try {
    GL_REQUIRE(public_inputs_hash, GL_ERR_ARG, "gl_prove_device_hashed: null hash");
    return prove_impl(ctx, cir, d_wires, nullptr, h_pis, npis, public_inputs_hash, out);
} catch (...) { return gl_caught(); }
// One pass of the proving pipeline over an all-zero witness, result thrown away: afterwards this context holds everything a proof of this
// circuit needs besides its own data -- the code objects of every kernel on the path loaded, the twiddle / power tables of the circuit's
// transform sizes built, the context's pool grown to the pipeline's working set.  (The reference precomputes its fft_root_table in build()
// too, circuit_builder.rs:1016-1019.)  A zero witness does not satisfy the circuit; nothing on the path asserts that it does.
extern "C" int gl_circuit_warm_up(gl_ctx* ctx, const gl_circuit* cir) try {
    GL_REQUIRE(ctx && cir, GL_ERR_ARG, "gl_circuit_warm_up: null argument");
    GL_REQUIRE(cir->ctx->device == ctx->device, GL_ERR_ARG, "gl_circuit_warm_up: circuit lives on another device");
    GL_TRY(ctx->activate());
    const size_t n = cir->n;
    DevBuf d_w(ctx); GL_TRY(d_w.alloc(135 * n * sizeof(gl_t)));
    GL_CHECK_HIP(hipMemsetAsync(d_w.p, 0, 135 * n * sizeof(gl_t), ctx->stream));
    std::vector<uint64_t> pis(cir->desc.num_public_inputs ? cir->desc.num_public_inputs : 1, 0);
    gl_proof* pr = nullptr;
    const int st = prove_impl(ctx, cir, d_w.as<gl_t>(), nullptr, pis.data(), cir->desc.num_public_inputs, nullptr, &pr);
    if (pr) gl_proof_free(pr);
    return st == GL_ERR_ZETA_IN_SUBGROUP ? GL_OK : st;       // (probability 2^-49: still warmed up to the opening point)
} catch (...) { return gl_caught(); }

extern "C" int gl_ctx_capture_intermediates(gl_ctx* ctx, int enable) try {
    GL_REQUIRE(ctx, GL_ERR_ARG, "null context");
    ctx->capture_intermediates = enable != 0;
    return GL_OK;
} catch (...) { return gl_caught(); }
