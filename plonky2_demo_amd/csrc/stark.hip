// The STARK prover's seam (starky/src/prover.rs, permutation.rs, stark.rs): an AIR handed over as data -- gl_stark_desc, one term
// list per constraint -- its validation, and the two prover phases the Plonk path has no counterpart for: the permutation
// argument's Z polynomials and the quotient (sum alpha^i C_i) / Z_H on the quotient coset.  Commitments, transforms and openings are
// the existing PolynomialBatch code; nothing is copied from it.
#include "context.hpp"
#include "fri_instance.hpp"
#include "openings_stage.hpp"
#include "proof.hpp"
#include "stark_internal.hpp"
#include "stark_kernels.cuh"
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace glstark;

glstark::StarkInstance::StarkInstance(uint32_t num_columns, uint32_t num_challenges, const StarkShape& s, uint32_t nctl, uint32_t degree_bits, gl2_t zeta) {
    ::memset((void*)&inst, 0, sizeof inst);
    const uint32_t nzs = s.nz + nctl, nq = s.q * num_challenges;
    uint32_t o = 0;
    const uint32_t trace_o = o; inst.oracle_num_polys[o++] = num_columns;
    const uint32_t zs_o = o; if (nzs) inst.oracle_num_polys[o++] = nzs;
    const uint32_t quot_o = o; inst.oracle_num_polys[o++] = nq;
    inst.num_oracles = o;
    inst.num_batches = nctl ? 3 : 2;
    const gl_t g = gl_host_root_of_unity(degree_bits);
    const gl2_t zeta_next = gl2_canon(gl2_scalar(zeta, g));
    inst.points[0][0] = zeta.a; inst.points[0][1] = zeta.b; inst.points[1][0] = zeta_next.a; inst.points[1][1] = zeta_next.b;
    polys.reserve(2 * (2 * (size_t)num_columns + 2 * nzs + nq + nctl));
    if (nctl) inst.points[2][0] = gl_canon(gl_inv(g));
    for (int b = 0; b < 2; b++) {
        const size_t before = polys.size() / 2;
        for (uint32_t c = 0; c < num_columns; c++) { polys.push_back(trace_o); polys.push_back(c); }
        for (uint32_t c = 0; c < nzs; c++) { polys.push_back(zs_o); polys.push_back(c); }
        if (b == 0) for (uint32_t c = 0; c < nq; c++) { polys.push_back(quot_o); polys.push_back(c); }
        inst.batch_len[b] = (uint32_t)(polys.size() / 2 - before);
    }
    for (uint32_t c = 0; c < nctl; c++) { polys.push_back(zs_o); polys.push_back(s.nz + c); }
    inst.batch_len[2] = nctl;
    inst.polys = polys.data();
}

int glstark::stark_check(const gl_stark_desc* desc, const gl_fri_params* params, StarkShape* shape, bool prover, const gl_stark_dag* dag, DagProgram* prog) {
    GL_REQUIRE(desc && params, GL_ERR_ARG, "gl_stark: null description / params");
    const gl_stark_desc& d = *desc;
    GL_REQUIRE(d.num_columns >= 1 && d.num_columns <= GL_STARK_MAX_COLUMNS, GL_ERR_ARG, "gl_stark: 1..1024 columns");
    GL_REQUIRE(d.num_public_inputs <= GL_STARK_MAX_PUBLIC_INPUTS, GL_ERR_ARG, "gl_stark: at most 256 public inputs");
    GL_REQUIRE(d.constraint_degree >= 1 && d.constraint_degree <= GL_STARK_MAX_DEGREE, GL_ERR_ARG, "gl_stark: constraint degree is 1..9");
    GL_REQUIRE(d.num_challenges >= 1 && d.num_challenges <= GL_STARK_MAX_CHALLENGES, GL_ERR_ARG, "gl_stark: 1..4 challenges");
    if (dag) {          // one form or the other per table
        GL_REQUIRE(!d.num_constraints && !d.constraint_filter && !d.constraint_num_terms && !d.term_coeff && !d.term_num_factors && !d.factors, GL_ERR_ARG,
                   "gl_stark_dag: the description carries a term list as well (num_constraints = 0 and null term tables go with a dag)");
    } else {
        GL_REQUIRE(d.num_constraints >= 1 && d.num_constraints <= GL_STARK_MAX_CONSTRAINTS, GL_ERR_ARG, "gl_stark: 1..4096 constraints");
        GL_REQUIRE(d.constraint_filter && d.constraint_num_terms && d.term_coeff && d.term_num_factors && d.factors, GL_ERR_ARG, "gl_stark: null constraint table");
    }
    GL_REQUIRE(d.num_permutation_pairs <= GL_STARK_MAX_PAIRS, GL_ERR_ARG, "gl_stark: at most 64 permutation pairs");
    GL_REQUIRE(!d.num_permutation_pairs || (d.pair_len && d.pair_columns), GL_ERR_ARG, "gl_stark: null permutation pair table");
    if (dag) GL_TRY(dag_compile(desc, dag, prog));
    StarkShape s;
    s.q = d.constraint_degree > 2 ? d.constraint_degree - 1 : 1;                 // stark.rs:79-81
    while ((1u << s.qdb) < s.q) s.qdb++;                                         // log2_ceil
    s.num_instances = d.num_permutation_pairs * d.num_challenges;
    s.nz = (s.num_instances + s.q - 1) / s.q;                                    // stark.rs:216-221
    for (uint32_t c = 0; c < d.num_constraints; c++) {
        const uint32_t filt = d.constraint_filter[c];
        GL_REQUIRE(filt <= GL_STARK_LAST_ROW, GL_ERR_ARG, "gl_stark: unknown constraint filter");
        GL_REQUIRE(d.constraint_num_terms[c] <= GL_STARK_MAX_TERMS - s.terms, GL_ERR_ARG, "gl_stark: more than 65536 terms");
        // quotient degree < q n: a term of k trace factors has degree k (n - 1); a row filter adds n - 1, the transition filter 1
        const uint32_t max_factors = (filt == GL_STARK_FIRST_ROW || filt == GL_STARK_LAST_ROW) ? s.q : s.q + 1;
        for (uint32_t t = 0; t < d.constraint_num_terms[c]; t++, s.terms++) {
            const uint32_t nf = d.term_num_factors[s.terms];
            GL_REQUIRE(nf <= GL_STARK_MAX_FACTORS, GL_ERR_ARG, "gl_stark: a term has more than 64 factors");
            uint32_t trace_factors = 0;
            for (uint32_t k = 0; k < nf; k++, s.factors++) {
                const uint32_t w = d.factors[s.factors], kind = w >> 30, idx = w & 0x3FFFFFFFu;
                GL_REQUIRE(kind <= GL_STARK_PUBLIC, GL_ERR_ARG, "gl_stark: unknown operand kind");
                if (kind == GL_STARK_PUBLIC) GL_REQUIRE(idx < d.num_public_inputs, GL_ERR_ARG, "gl_stark: public-input index out of range");
                else { GL_REQUIRE(idx < d.num_columns, GL_ERR_ARG, "gl_stark: column index out of range"); trace_factors++; }
            }
            GL_REQUIRE(trace_factors <= max_factors, GL_ERR_ARG, "gl_stark: a term's degree is above the constraint degree (too many LOCAL / NEXT factors)");
        }
    }
    for (uint32_t pr = 0; pr < d.num_permutation_pairs; pr++) {
        GL_REQUIRE(d.pair_len[pr] >= 1 && d.pair_len[pr] <= GL_STARK_MAX_PAIR_LEN, GL_ERR_ARG, "gl_stark: a permutation pair has 1..64 column pairs");
        for (uint32_t k = 0; k < 2 * d.pair_len[pr]; k++)
            GL_REQUIRE(d.pair_columns[2 * s.column_pairs + k] < d.num_columns, GL_ERR_ARG, "gl_stark: permutation column out of range");
        s.column_pairs += d.pair_len[pr];
    }
    GL_REQUIRE(params->hiding == 0, GL_ERR_UNSUPPORTED, "gl_stark: hiding is not supported (StarkConfig::fri_params passes false)");
    // the gl_fri_params rules are gl_prove_openings' own, on the STARK's instance (an opening point off the base field passes its coset check)
    const StarkInstance si(d.num_columns, d.num_challenges, s, 0, params->degree_bits);
    GL_TRY(glfri::check(params, &si.inst, prover));
    GL_REQUIRE(s.qdb <= params->rate_bits, GL_ERR_UNSUPPORTED, "gl_stark: constraints of degree higher than the rate are not supported (prover.rs:222-225)");
    if (shape) *shape = s;
    return GL_OK;
}


extern "C" int gl_stark_check(const gl_stark_desc* desc, const gl_fri_params* params) try {
    return stark_check(desc, params, nullptr);
} catch (...) { return gl_caught(); }

extern "C" void gl_stark_free(gl_stark* s) noexcept {
    if (!s) return;
    if (s->ctx) {
        if (s->d_tables) s->ctx->pool_release(s->d_tables);
        if (s->d_lagrange) s->ctx->pool_release(s->d_lagrange);
        gl_ctx_release(s->ctx);
    }
    delete s;
}

extern "C" int gl_stark_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_fri_params* params, gl_stark** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_stark_create: null out");
    *out = nullptr;
    return stark_create(ctx, desc, nullptr, params, out);
} catch (...) { return gl_caught(); }

// gl_stark_create and gl_stark_dag_create: with a dag its compiled program stands in the tables where the term program would
int glstark::stark_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, gl_stark** out) {
    GL_REQUIRE(ctx, GL_ERR_ARG, "gl_stark_create: null context");
    StarkShape sh;
    DagProgram prog;
    GL_TRY(stark_check(desc, params, &sh, true, dag, &prog));
    GL_TRY(ctx->activate());
    const gl_stark_desc& d = *desc;
    std::unique_ptr<gl_stark, void (*)(gl_stark*)> s(new gl_stark(), gl_stark_free);
    s->ctx = ctx; ctx->retain();
    s->params = *params; s->s = sh;
    s->num_columns = d.num_columns; s->num_public_inputs = d.num_public_inputs; s->nc = d.num_challenges; s->num_constraints = d.num_constraints;
    s->n = size_t(1) << params->degree_bits; s->size = s->n << sh.qdb;
    s->proof_bytes = table_proof_bytes(*params, d.num_columns, d.num_public_inputs, d.num_challenges, sh, 0);
    const uint32_t lgS = params->degree_bits + sh.qdb, nzh = 1u << sh.qdb;
    // per-degree_bits constants: g^-1, 1/n, Z_H and 1/Z_H on the coset (ZeroPolyOnCoset, field/src/zero_poly_coset.rs:19-36)
    s->last = gl_canon(gl_inv(gl_host_root_of_unity(params->degree_bits)));
    s->n_inv = gl_host_inverse_2exp(params->degree_bits);
    gl_t zh[8] = {0};
    {
        gl_t g_pow_n = GL_MULT_GENERATOR; for (uint32_t i = 0; i < params->degree_bits; i++) g_pow_n = gl_sqr(g_pow_n);
        gl_t w = gl_host_root_of_unity(sh.qdb), x = 1;
        for (uint32_t i = 0; i < nzh; i++) { zh[i] = gl_canon(gl_sub(gl_mul(g_pow_n, x), 1)); s->zh_inv[i] = gl_canon(gl_inv(zh[i])); x = gl_mul(x, w); }
    }
    // one host image of the tables, 8-byte words first
    const size_t npairs = d.num_permutation_pairs;
    const size_t nconst = prog.constants.size();
    std::vector<gl_t> words(sh.terms + nconst + 8);
    for (size_t t = 0; t < sh.terms; t++) words[t] = gl_canon(d.term_coeff[t]);
    for (size_t i = 0; i < nconst; i++) words[sh.terms + i] = prog.constants[i];
    for (uint32_t i = 0; i < 8; i++) words[sh.terms + nconst + i] = zh[i];
    std::vector<uint32_t> u32;
    const size_t o_filter = 0, o_num_terms = o_filter + d.num_constraints, o_term_nf = o_num_terms + d.num_constraints, o_factors = o_term_nf + sh.terms,
                 o_pair_off = o_factors + sh.factors, o_pair_cols = o_pair_off + npairs + 1, end32 = o_pair_cols + 2 * sh.column_pairs,
                 o_dag = end32 + ((4 - (2 * words.size() + end32) % 4) % 4),       // the compiled DAG on a 16-byte boundary of the block
                 total32 = o_dag + prog.instr.size();
    u32.resize(total32 + 2);
    for (uint32_t c = 0; c < d.num_constraints; c++) { u32[o_filter + c] = d.constraint_filter[c]; u32[o_num_terms + c] = d.constraint_num_terms[c]; }
    for (size_t t = 0; t < sh.terms; t++) u32[o_term_nf + t] = d.term_num_factors[t];
    for (size_t f = 0; f < sh.factors; f++) u32[o_factors + f] = d.factors[f];
    uint32_t off = 0;
    for (size_t pr = 0; pr < npairs; pr++) { u32[o_pair_off + pr] = off; off += d.pair_len[pr]; }
    u32[o_pair_off + npairs] = off;
    for (size_t k = 0; k < 2 * sh.column_pairs; k++) u32[o_pair_cols + k] = d.pair_columns[k];
    for (size_t k = 0; k < prog.instr.size(); k++) u32[o_dag + k] = prog.instr[k];
    const size_t bytes64 = words.size() * sizeof(gl_t), bytes32 = u32.size() * sizeof(uint32_t);
    GL_TRY(ctx->pool_alloc(bytes64 + bytes32, &s->d_tables));
    GL_TRY(gl_copy_h2d(ctx, s->d_tables, words.data(), bytes64));
    GL_TRY(gl_copy_h2d(ctx, (char*)s->d_tables + bytes64, u32.data(), bytes32));
    s->d_coeff = (const gl_t*)s->d_tables;
    const gl_t* d_zh = s->d_coeff + sh.terms + nconst;
    s->dag = dag != nullptr; s->d_dag_const = s->d_coeff + sh.terms;
    s->dag_num_instructions = prog.num_instructions; s->dag_max_live = prog.max_live;
    const uint32_t* d32 = (const uint32_t*)((const char*)s->d_tables + bytes64);
    s->d_filter = d32 + o_filter; s->d_num_terms = d32 + o_num_terms; s->d_term_nf = d32 + o_term_nf; s->d_factors = d32 + o_factors;
    s->d_pair_off = d32 + o_pair_off; s->d_pair_cols = d32 + o_pair_cols; s->d_dag_instr = d32 + o_dag;
    GL_TRY(ctx->get_pow_table(gl_host_root_of_unity(lgS), GL_MULT_GENERATOR, (uint32_t)((s->size + 2047) >> 11), &s->xt));
    GL_TRY(ctx->pool_alloc(2 * s->size * sizeof(gl_t), (void**)&s->d_lagrange));
    hipLaunchKernelGGL(k_stark_lagrange_on_coset, dim3((unsigned)((s->size + 255) / 256)), dim3(256), 0, ctx->stream, s->xt.lo, s->xt.hi, (uint32_t)s->size,
                       nzh - 1, d_zh, s->n_inv, s->last, s->d_lagrange, s->d_lagrange + s->size);
    GL_CHECK_HIP(hipGetLastError());
    GL_CHECK_HIP(gl_stream_wait(ctx->stream));
    *out = s.release();
    return GL_OK;
}

namespace {

int check_stark_args(gl_ctx* ctx, const gl_stark* s) {
    GL_REQUIRE(ctx && s, GL_ERR_ARG, "gl_stark: null context / stark");
    // the tables are blocks of the creating context's stream-ordered pool: only that context's stream orders their use and their release
    GL_REQUIRE(s->ctx == ctx, GL_ERR_ARG, "gl_stark: the stark was created on another context");
    return ctx->activate();
}

}  // namespace

int glstark::check_stark_batch(const gl_stark* s, const gl_batch* b, size_t ncols, const char* what) {
    GL_REQUIRE(b && b->ncols == ncols && b->n == s->n && b->rate_bits == s->params.rate_bits && b->cap_height == s->params.cap_height && b->salt == 0, GL_ERR_ARG, what);
    GL_REQUIRE(b->hasher == s->params.hasher, GL_ERR_ARG, "gl_stark: a batch committed under another hasher than the params'");
    return GL_OK;
}
// the challenge sets [q][num_challenges][2], canonical, into a pool block (synchronises: the host source is the caller's)
int glstark::upload_challenges(gl_ctx* ctx, const gl_stark* s, const uint64_t* challenges, DevBuf& d_ch) {
    std::vector<gl_t> ch((size_t)s->s.q * s->nc * 2);
    for (size_t i = 0; i < ch.size(); i++) ch[i] = gl_canon(challenges[i]);
    GL_TRY(d_ch.alloc(ch.size() * sizeof(gl_t)));
    return gl_copy_h2d(ctx, d_ch.p, ch.data(), ch.size() * sizeof(gl_t));
}
int glstark::read_flag(gl_ctx* ctx, const uint32_t* d_flag, uint32_t* flag) { return gl_copy_d2h(ctx, flag, d_flag, sizeof *flag); }

// compute_permutation_z_polys (permutation.rs:66-117): d_trace VALUES [num_columns][n] -> d_z VALUES [nz][n]
int glstark::permutation_z_values(gl_ctx* ctx, const gl_stark* s, const gl_t* d_trace, const gl_t* d_ch, gl_t* d_z) {
    const uint32_t n = (uint32_t)s->n, nz = s->s.nz, nseg = (n + GLS_SEG - 1) / GLS_SEG;
    hipStream_t st = ctx->stream;
    DevBuf d_quot(ctx), d_seg(ctx), d_flag(ctx);
    GL_TRY(d_quot.alloc((size_t)nz * n * sizeof(gl_t)));
    GL_TRY(d_seg.alloc((size_t)nz * nseg * sizeof(gl_t)));
    GL_TRY(d_flag.alloc(sizeof(uint32_t)));
    GL_CHECK_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), st));
    GlStarkPerm p;
    p.trace = d_trace; p.ch = d_ch; p.pair_off = s->d_pair_off; p.pair_cols = s->d_pair_cols;
    p.n = n; p.q = s->s.q; p.nc = s->nc; p.num_instances = s->s.num_instances;
    ctx->timing_begin("compute permutation Z polys");
    hipLaunchKernelGGL(k_stark_perm_quotients, dim3(nseg, nz), dim3(256), 0, st, p, d_quot.as<gl_t>(), d_flag.as<uint32_t>());
    hipLaunchKernelGGL(k_stark_seg_products, dim3(nseg, nz), dim3(256), 0, st, d_quot.as<const gl_t>(), n, d_seg.as<gl_t>());
    hipLaunchKernelGGL(k_stark_seg_scan, dim3((nz + 63) / 64), dim3(64), 0, st, d_seg.as<gl_t>(), nseg, nz);
    hipLaunchKernelGGL(k_stark_z_finalize, dim3(nseg, nz), dim3(256), 0, st, d_quot.as<const gl_t>(), d_seg.as<const gl_t>(), n, d_z);
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    uint32_t flag = 0;
    GL_TRY(read_flag(ctx, d_flag.as<uint32_t>(), &flag));
    GL_REQUIRE(!flag, GL_ERR_ARG, "gl_stark: a permutation denominator is zero under these challenges (probability about n / p)");
    return GL_OK;
}

namespace {

// compute_quotient_polys up to the coset_ifft (prover.rs:198-311): d_out[num_challenges][size] values on the quotient coset
int quotient_values(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const gl_t* d_ch, const uint64_t* alphas, const gl_t* d_pub, gl_t* d_out) {
    if (s->dag) return quotient_dag_launch(ctx, s, trace, zs, d_ch, alphas, d_pub, d_out);      // k_stark_quotient_dag (stark_dag.hip)
    GlStarkQuot q;
    ::memset((void*)&q, 0, sizeof q);
    q.trace = trace->lde; q.zs = zs ? zs->lde : nullptr; q.stride = trace->N();
    q.filter = s->d_filter; q.num_terms = s->d_num_terms; q.term_nf = s->d_term_nf; q.factors = s->d_factors; q.coeff = s->d_coeff;
    q.pub = d_pub; q.ch = d_ch; q.pair_off = s->d_pair_off; q.pair_cols = s->d_pair_cols;
    q.xpow_lo = s->xt.lo; q.xpow_hi = s->xt.hi; q.lfirst = s->d_lagrange; q.llast = s->d_lagrange + s->size; q.out = d_out;
    for (uint32_t j = 0; j < s->nc; j++) q.alphas[j] = gl_canon(alphas[j]);
    for (int i = 0; i < 8; i++) q.zh_inv[i] = s->zh_inv[i];
    q.last = s->last;
    q.size = (uint32_t)s->size; q.step = 1u << (s->params.rate_bits - s->s.qdb); q.next_step = 1u << s->s.qdb;
    q.num_constraints = s->num_constraints; q.nc = s->nc; q.q = s->s.q; q.nz = zs ? s->s.nz : 0; q.num_instances = s->s.num_instances;
    const dim3 grid((unsigned)((s->size + 255) / 256)), block(256);
    ctx->timing_begin("compute quotient polys");
    switch (s->nc) {
        case 1: hipLaunchKernelGGL(k_stark_quotient<1>, grid, block, 0, ctx->stream, q); break;
        case 2: hipLaunchKernelGGL(k_stark_quotient<2>, grid, block, 0, ctx->stream, q); break;
        case 3: hipLaunchKernelGGL(k_stark_quotient<3>, grid, block, 0, ctx->stream, q); break;
        default: hipLaunchKernelGGL(k_stark_quotient<4>, grid, block, 0, ctx->stream, q); break;
    }
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}

}  // namespace

// what the quotient entries share: argument checks, the uploads, the kernel and a set's CTL pass behind it; d_q[num_challenges][size]
int glstark::quotient_phase(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges, const uint64_t* alphas,
                   const uint64_t* public_inputs, DevBuf& d_q, const TableCtl* ctl) {
    const uint32_t nz = s ? s->s.nz : 0, nctl = nctl_of(ctl);
    GL_TRY(check_stark_args(ctx, s));
    GL_REQUIRE(alphas && (public_inputs || !s->num_public_inputs), GL_ERR_ARG, "gl_stark quotient: null alphas / public inputs");
    GL_TRY(check_stark_batch(s, trace, s->num_columns, "gl_stark quotient: the trace batch does not match the description / params"));
    GL_REQUIRE((nz + nctl != 0) == (zs != nullptr) && (nz == 0 || challenges), GL_ERR_ARG,
               "gl_stark quotient: the Z batch and the challenge sets go with permutation pairs (null without)");
    if (zs) GL_TRY(check_stark_batch(s, zs, nz + nctl, "gl_stark quotient: the Z batch does not match the description / params"));   // a set's: CTL Zs follow
    DevBuf d_ch(ctx), d_pub(ctx);
    if (nz) GL_TRY(upload_challenges(ctx, s, challenges, d_ch));
    std::vector<gl_t> pub(s->num_public_inputs + 1, 0);
    for (uint32_t i = 0; i < s->num_public_inputs; i++) pub[i] = gl_canon(public_inputs[i]);
    GL_TRY(d_pub.alloc(pub.size() * sizeof(gl_t)));
    GL_TRY(gl_copy_h2d(ctx, d_pub.p, pub.data(), pub.size() * sizeof(gl_t)));
    GL_TRY(d_q.alloc((size_t)s->nc * s->size * sizeof(gl_t)));
    GL_TRY(quotient_values(ctx, s, trace, nz ? zs : nullptr, d_ch.as<const gl_t>(), alphas, d_pub.as<const gl_t>(), d_q.as<gl_t>()));
    return nctl ? ctl_quotient_pass(ctx, *ctl, trace, zs, alphas, d_q) : GL_OK;
}

int glstark::zs_commit(gl_ctx* ctx, const gl_stark* s, const TableCtl* ctl, const uint64_t* d_trace_values, const uint64_t* challenges, gl_batch** zs) {
    const uint32_t nz = s->s.nz, nctl = nctl_of(ctl);
    DevBuf d_ch(ctx), d_z(ctx);
    GL_TRY(d_z.alloc((size_t)(nz + nctl) * s->n * sizeof(gl_t)));
    if (nz) {
        GL_TRY(upload_challenges(ctx, s, challenges, d_ch));
        GL_TRY(permutation_z_values(ctx, s, d_trace_values, d_ch.as<const gl_t>(), d_z.as<gl_t>()));
    }
    if (nctl) GL_TRY(ctl_z_values(ctx, *ctl, d_trace_values, d_z.as<gl_t>() + (size_t)nz * s->n));
    return gl_batch_from_device_h(ctx, s->params.hasher, d_z.as<uint64_t>(), nz + nctl, s->n, s->params.rate_bits, s->params.cap_height, 1, zs);
}

extern "C" int gl_stark_permutation_zs(gl_ctx* ctx, const gl_stark* s, const uint64_t* d_trace_values, const uint64_t* challenges, gl_batch** zs) try {
    GL_REQUIRE(zs, GL_ERR_ARG, "gl_stark_permutation_zs: null out");
    *zs = nullptr;
    GL_TRY(check_stark_args(ctx, s));
    GL_REQUIRE(d_trace_values && challenges, GL_ERR_ARG, "gl_stark_permutation_zs: null argument");
    GL_REQUIRE(s->s.nz, GL_ERR_ARG, "gl_stark_permutation_zs: the description has no permutation pairs");
    return zs_commit(ctx, s, nullptr, d_trace_values, challenges, zs);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_quotient_values(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges,
                                        const uint64_t* alphas, const uint64_t* public_inputs, uint64_t* h_out) try {
    GL_REQUIRE(h_out, GL_ERR_ARG, "gl_stark_quotient_values: null out");
    DevBuf d_q(ctx);
    GL_TRY(quotient_phase(ctx, s, trace, zs, challenges, alphas, public_inputs, d_q));
    return gl_copy_d2h(ctx, h_out, d_q.p, (size_t)s->nc * s->size * sizeof(gl_t));
} catch (...) { return gl_caught(); }

// the quotient's values d_q[num_challenges][size] on the coset -> the committed chunk polynomials (prover.rs:114-144)
int glstark::quotient_commit(gl_ctx* ctx, const gl_stark* s, DevBuf& d_q, gl_batch** quotient) {
    const uint32_t lgS = s->params.degree_bits + s->s.qdb, size = (uint32_t)s->size, keep = (uint32_t)(s->s.q * s->n);
    hipStream_t st = ctx->stream;
    // values.coset_ifft(F::coset_shift()) (prover.rs:313-317)
    GL_TRY(gl_ntt_run(ctx, d_q.as<gl_t>(), size, size, d_q.as<gl_t>(), size, lgS, s->nc, true, 0, gl_canon(gl_inv(GL_MULT_GENERATOR)), gl_host_inverse_2exp(lgS)));
    if (keep < size) {          // trim_to_len(quotient_degree_factor * degree) (prover.rs:123-128): q is no power of two
        DevBuf d_flag(ctx);
        GL_TRY(d_flag.alloc(sizeof(uint32_t)));
        GL_CHECK_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_stark_tail_nonzero, dim3((size - keep + 255) / 256, s->nc), dim3(256), 0, st, d_q.as<const gl_t>(), size, keep, d_flag.as<uint32_t>());
        GL_CHECK_HIP(hipGetLastError());
        uint32_t flag = 0;
        GL_TRY(read_flag(ctx, d_flag.as<uint32_t>(), &flag));
        GL_REQUIRE(!flag, GL_ERR_ARG, "gl_stark: the trace does not satisfy the constraints (the quotient's degree is too high)");
    }
    // chunks of n coefficients, challenge after challenge (prover.rs:129-131), committed from coefficients
    DevBuf d_c(ctx);
    GL_TRY(d_c.alloc((size_t)s->nc * keep * sizeof(gl_t)));
    for (uint32_t j = 0; j < s->nc; j++)
        GL_CHECK_HIP(hipMemcpyAsync(d_c.as<gl_t>() + (size_t)j * keep, d_q.as<gl_t>() + (size_t)j * size, (size_t)keep * sizeof(gl_t), hipMemcpyDeviceToDevice, st));
    return gl_batch_from_device_h(ctx, s->params.hasher, d_c.as<uint64_t>(), (size_t)s->nc * s->s.q, s->n, s->params.rate_bits, s->params.cap_height, 0, quotient);
}

extern "C" int gl_stark_quotient_polys(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges,
                                       const uint64_t* alphas, const uint64_t* public_inputs, gl_batch** quotient) try {
    GL_REQUIRE(quotient, GL_ERR_ARG, "gl_stark_quotient_polys: null out");
    *quotient = nullptr;
    DevBuf d_q(ctx);
    GL_TRY(quotient_phase(ctx, s, trace, zs, challenges, alphas, public_inputs, d_q));
    return quotient_commit(ctx, s, d_q, quotient);
} catch (...) { return gl_caught(); }

// ---- the whole prover and the verifier (starky/src/prover.rs:32-194, verifier.rs:21-145) -------------------------------------------
size_t glstark::table_proof_bytes(const gl_fri_params& p, uint32_t num_columns, uint32_t num_public_inputs, uint32_t nc, const StarkShape& s, uint32_t nctl) {
    const StarkInstance si(num_columns, nc, s, nctl, p.degree_bits);
    return si.inst.num_oracles * (hash_wire_bytes(p.hasher) << p.cap_height) + 16 * (2 * (size_t)num_columns + 2 * (size_t)(s.nz + nctl) + (size_t)s.q * nc) +
           8 * (size_t)nctl + glfri::proof_bytes(p, si.inst) + 8 * (size_t)num_public_inputs;
}
gl2_t glstark::ext_pow2(gl2_t x, unsigned k) { for (unsigned i = 0; i < k; i++) x = gl2_mul(x, x); return gl2_canon(x); }

int glstark::prove_table(gl_ctx* ctx, const gl_stark* s, const TableCtl* ctl, const uint64_t* d_cols, const gl_batch* trace, const uint64_t* h_public_inputs,
                         gl_challenger& ch, std::vector<uint8_t>& o, const char* who) {
    const gl_fri_params& p = s->params;
    const size_t ncap = size_t(1) << p.cap_height, start = o.size() - hash_wire_bytes(p.hasher) * ncap;      // where the trace cap stands
    const uint32_t nz = s->s.nz, nctl = nctl_of(ctl), nzs = nz + nctl, nq = s->s.q * s->nc, ncols = s->num_columns;
    auto fail = [&](int code, const char* what) { return gl_fail(code, (std::string(who) + what).c_str(), __FILE__, __LINE__); };
    std::vector<gl_t> cap(4 * ncap);
    BatchHolder zs, quot;
    // permutation challenge sets, the Z polynomials (a set's CTL Zs behind them), their commitment (prover.rs:76-111)
    std::vector<gl_t> sets;
    if (nz) for (uint32_t i = 0; i < 2 * s->s.q * s->nc; i++) sets.push_back(ch.ch.challenge());          // set after set: (beta, gamma) per challenge
    if (nzs) {
        GL_TRY(zs_commit(ctx, s, ctl, d_cols, nz ? sets.data() : nullptr, &zs.b));
        GL_TRY(gl_batch_cap(zs.b, cap.data()));
        put_hashes(o, p.hasher, cap.data(), ncap);
        ch.ch.observe_hashes(p.hasher, cap.data(), ncap);
    }
    // alphas, the quotient, its commitment (prover.rs:113-146)
    gl_t alphas[GL_STARK_MAX_CHALLENGES];
    for (uint32_t j = 0; j < s->nc; j++) alphas[j] = ch.ch.challenge();
    {
        DevBuf d_q(ctx);
        GL_TRY(quotient_phase(ctx, s, trace, zs.b, nz ? sets.data() : nullptr, alphas, h_public_inputs, d_q, ctl));
        GL_TRY(quotient_commit(ctx, s, d_q, &quot.b));
    }
    GL_TRY(gl_batch_cap(quot.b, cap.data()));
    put_hashes(o, p.hasher, cap.data(), ncap);
    ch.ch.observe_hashes(p.hasher, cap.data(), ncap);
    // zeta off the subgroup (prover.rs:148-157); the instance holds zeta, g zeta and g^-1
    const gl2_t zeta = ch.ch.challenge_ext();
    const gl2_t zn = ext_pow2(zeta, p.degree_bits);
    if (zn.a == 1 && zn.b == 0) return fail(GL_ERR_ZETA_IN_SUBGROUP, ": opening point is in the subgroup");
    const StarkInstance si(ncols, s->nc, s->s, nctl, p.degree_bits, zeta);
    const uint64_t *zw = si.inst.points[0], *znw = si.inst.points[1], *lw = si.inst.points[2];
    // StarkOpeningSet::new (proof.rs:138-159, evm/src/proof.rs:224-259)
    std::vector<gl_t> local(2 * ncols), next(2 * ncols), zl(2 * nzs), zn_(2 * nzs), last(2 * nctl), ql(2 * nq);
    GL_TRY(gl_open_at(ctx, trace, zw, 0, ncols, local.data()));
    GL_TRY(gl_open_at(ctx, trace, znw, 0, ncols, next.data()));
    if (nzs) { GL_TRY(gl_open_at(ctx, zs.b, zw, 0, nzs, zl.data())); GL_TRY(gl_open_at(ctx, zs.b, znw, 0, nzs, zn_.data())); }
    if (nctl) GL_TRY(gl_open_at(ctx, zs.b, lw, nz, nctl, last.data()));
    GL_TRY(gl_open_at(ctx, quot.b, zw, 0, nq, ql.data()));
    for (uint32_t k = 0; k < nctl; k++) if (gl_canon(last[2 * k + 1]) != 0) return fail(GL_ERR_INTERNAL, ": a base-field opening left the base field");
    put_words(o, local.data(), local.size()); put_words(o, next.data(), next.size());
    put_words(o, zl.data(), zl.size()); put_words(o, zn_.data(), zn_.size());
    for (uint32_t k = 0; k < nctl; k++) put_u64(o, gl_canon(last[2 * k]));
    put_words(o, ql.data(), ql.size());
    // observe_openings(to_fri_openings) (proof.rs:161-182): [local, zs, quotient] at zeta, [next, zs_next] at g zeta, [ctl_zs_last lifted] at g^-1
    ch.ch.observe_many(local.data(), local.size()); ch.ch.observe_many(zl.data(), zl.size()); ch.ch.observe_many(ql.data(), ql.size());
    ch.ch.observe_many(next.data(), next.size()); ch.ch.observe_many(zn_.data(), zn_.size());
    ch.ch.observe_many(last.data(), last.size());
    // prove_openings on the table's instance (prover.rs:172-186)
    const gl_batch* batches[3] = {trace, nzs ? zs.b : quot.b, quot.b};
    const size_t at = o.size(), fri_len = glfri::proof_bytes(p, si.inst);
    size_t fri_bytes = 0;
    o.resize(at + fri_len);
    GL_TRY(gl_prove_openings(ctx, &p, &si.inst, batches, &ch, o.data() + at, fri_len, &fri_bytes));
    if (fri_bytes != fri_len) return fail(GL_ERR_INTERNAL, ": the FriProof has another size than the params and the instance fix");
    for (uint32_t i = 0; i < s->num_public_inputs; i++) put_u64(o, gl_canon(h_public_inputs[i]));
    if (o.size() - start != table_proof_bytes(p, ncols, s->num_public_inputs, s->nc, s->s, nctl))
        return fail(GL_ERR_INTERNAL, ": a table's proof has another size than the description and the params fix");
    return GL_OK;
}

namespace {

int stark_prove_device(gl_ctx* ctx, const gl_stark* s, const uint64_t* d_cols, const uint64_t* h_public_inputs, uint8_t* h_out, size_t cap_bytes, size_t* num_bytes) {
    GL_TRY(check_stark_args(ctx, s));
    GL_REQUIRE(d_cols && num_bytes && (h_public_inputs || !s->num_public_inputs), GL_ERR_ARG, "gl_stark_prove: null argument");
    const gl_fri_params& p = s->params;
    const size_t total = gl_stark_proof_size(s), ncap = size_t(1) << p.cap_height;
    *num_bytes = total;
    GL_REQUIRE(h_out && cap_bytes >= total, GL_ERR_ARG, "gl_stark_prove: output too small (gl_stark_proof_size)");
    std::vector<uint8_t> o;
    o.reserve(total);
    gl_challenger ch{glhost::HostChallenger(p.hasher)};
    std::vector<gl_t> cap(4 * ncap);
    BatchHolder trace;
    // the trace commitment (prover.rs:52-68), then the table's body
    GL_TRY(gl_batch_from_device_h(ctx, p.hasher, d_cols, s->num_columns, s->n, p.rate_bits, p.cap_height, 1, &trace.b));
    GL_TRY(gl_batch_cap(trace.b, cap.data()));
    put_hashes(o, p.hasher, cap.data(), ncap);
    ch.ch.observe_hashes(p.hasher, cap.data(), ncap);
    GL_TRY(prove_table(ctx, s, nullptr, d_cols, trace.b, h_public_inputs, ch, o, "gl_stark_prove"));
    GL_REQUIRE(o.size() == total, GL_ERR_INTERNAL, "gl_stark_prove: the proof has another size than gl_stark_proof_size");
    ::memcpy(h_out, o.data(), total);
    return GL_OK;
}

}  // namespace

int glstark::stark_reject(uint32_t code, uint32_t* check) {
    if (check) *check = code;
    return gl_fail(GL_ERR_VERIFY, gl_verify_check_message(code), __FILE__, __LINE__);
}

// eval_vanishing_poly at zeta over the extension field (vanishing_poly.rs, verifier.rs:81-106): the host interpreter of the term list
void glstark::vanishing_at(const gl_stark_desc& d, const StarkShape& s, const gl2_t* local, const gl2_t* next, const gl_t* pub, const gl_t* alphas, gl2_t z_last,
                  gl2_t l_first, gl2_t l_last, const gl2_t* zs, const gl2_t* zs_next, const gl_t* sets, gl2_t* accs, const DagProgram* prog, const TableCtl* ctl) {
    const uint32_t nc = d.num_challenges;
    for (uint32_t j = 0; j < nc; j++) accs[j] = gl2_make(0, 0);
    auto consume = [&](gl2_t c) { for (uint32_t j = 0; j < nc; j++) accs[j] = gl2_add(gl2_scalar(accs[j], alphas[j]), c); };
    size_t t = 0, f = 0;
    for (uint32_t c = 0; c < d.num_constraints; c++) {
        gl2_t C = gl2_make(0, 0);
        for (uint32_t k = 0; k < d.constraint_num_terms[c]; k++, t++) {
            gl2_t m = e_of(d.term_coeff[t]);
            for (uint32_t x = 0; x < d.term_num_factors[t]; x++, f++) {
                const uint32_t w = d.factors[f], kind = w >> 30, idx = w & 0x3FFFFFFFu;
                m = gl2_mul(m, kind == GL_STARK_LOCAL ? local[idx] : kind == GL_STARK_NEXT ? next[idx] : e_of(pub[idx]));
            }
            C = gl2_add(C, m);
        }
        const uint32_t filt = d.constraint_filter[c];
        consume(filt == GL_STARK_TRANSITION ? gl2_mul(C, z_last) : filt == GL_STARK_FIRST_ROW ? gl2_mul(C, l_first) : filt == GL_STARK_LAST_ROW ? gl2_mul(C, l_last) : C);
    }
    if (prog) dag_constraints_at(*prog, local, next, pub, z_last, l_first, l_last, consume);             // the other form: no term list above
    for (uint32_t b = 0; b < s.nz; b++) consume(gl2_mul(gl2_sub(zs[b], gl2_make(1, 0)), l_first));      // permutation.rs:282-285
    std::vector<uint32_t> pair_off(d.num_permutation_pairs + 1, 0);
    for (uint32_t pr = 0; pr < d.num_permutation_pairs; pr++) pair_off[pr + 1] = pair_off[pr] + d.pair_len[pr];
    for (uint32_t b = 0; b < s.nz; b++) {                                                                  // permutation.rs:296-320
        gl2_t pl = zs[b], prd = zs_next[b];
        for (uint32_t e = b * s.q; e < std::min(b * s.q + s.q, s.num_instances); e++) {
            const uint32_t pair = e / nc, chal = e % nc, j = e - b * s.q;
            const gl_t beta = sets[(j * nc + chal) * 2], gamma = sets[(j * nc + chal) * 2 + 1];
            gl2_t lhs = gl2_make(0, 0), rhs = gl2_make(0, 0);
            for (uint32_t k = d.pair_len[pair]; k-- > 0;) {
                lhs = gl2_add(gl2_scalar(lhs, beta), local[d.pair_columns[2 * (pair_off[pair] + k)]]);
                rhs = gl2_add(gl2_scalar(rhs, beta), local[d.pair_columns[2 * (pair_off[pair] + k) + 1]]);
            }
            pl = gl2_mul(pl, gl2_add(lhs, e_of(gamma)));
            prd = gl2_mul(prd, gl2_add(rhs, e_of(gamma)));
        }
        consume(gl2_sub(prd, pl));
    }
    if (nctl_of(ctl)) ctl_checks_at(*ctl, local, next, zs + s.nz, zs_next + s.nz, l_first, z_last, consume);      // the Zs after the permutation ones
}

extern "C" size_t gl_stark_proof_size(const gl_stark* s) noexcept {
    return s ? s->proof_bytes : 0;
}

extern "C" int gl_stark_prove_device(gl_ctx* ctx, const gl_stark* s, const uint64_t* d_cols, const uint64_t* h_public_inputs, uint8_t* h_out,
                                     size_t cap_bytes, size_t* num_bytes) try {
    return stark_prove_device(ctx, s, d_cols, h_public_inputs, h_out, cap_bytes, num_bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_prove(gl_ctx* ctx, const gl_stark* s, const uint64_t* const* h_trace_cols, const uint64_t* h_public_inputs, uint8_t* h_out,
                              size_t cap_bytes, size_t* num_bytes) try {
    GL_TRY(check_stark_args(ctx, s));
    GL_REQUIRE(h_trace_cols, GL_ERR_ARG, "gl_stark_prove: null trace");
    for (uint32_t c = 0; c < s->num_columns; c++) GL_REQUIRE(h_trace_cols[c], GL_ERR_ARG, "gl_stark_prove: null trace column");
    DevBuf d_cols(ctx);
    GL_TRY(d_cols.alloc((size_t)s->num_columns * s->n * sizeof(gl_t)));
    for (uint32_t c = 0; c < s->num_columns; c++)
        GL_CHECK_HIP(hipMemcpyAsync(d_cols.as<gl_t>() + (size_t)c * s->n, h_trace_cols[c], s->n * sizeof(gl_t), hipMemcpyHostToDevice, ctx->stream));
    GL_CHECK_HIP(gl_stream_wait(ctx->stream));          // pageable sources must not be reused before the copies land
    return stark_prove_device(ctx, s, d_cols.as<uint64_t>(), h_public_inputs, h_out, cap_bytes, num_bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_verify(const gl_stark_desc* desc, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check) try {
    if (check) *check = GL_CHECK_ACCEPTED;
    return stark_verify(desc, nullptr, params, proof_bytes, num_bytes, check);
} catch (...) { return gl_caught(); }

int glstark::stark_host_stage(const gl_stark_desc& d, const StarkShape& s, const DagProgram* prog, const gl_fri_params& p, const TableCtl* ctl, const uint8_t* proof_bytes,
                              size_t num_bytes, size_t total, gl_challenger& ch, StarkClaim& out, uint32_t* check) {
    if (check) *check = GL_CHECK_ACCEPTED;
    GL_REQUIRE(proof_bytes || !num_bytes, GL_ERR_ARG, "gl_stark_verify: null proof");
    const uint32_t nc = d.num_challenges, ncols = d.num_columns, nz = s.nz, nctl = nctl_of(ctl), nzs = nz + nctl, nq = s.q * nc;
    const size_t ncap = size_t(1) << p.cap_height;
    // the layout's counts are fixed by the description and the params (a set's are decided on the whole set's size before)
    if (num_bytes < total) return stark_reject(GL_CHECK_TRUNCATED, check);
    if (num_bytes > total) return stark_reject(GL_CHECK_LENGTH, check);
    VCursor cur{proof_bytes, num_bytes};
    const uint32_t noracles = nzs ? 3 : 2;
    std::vector<gl_t>& caps = out.caps;
    std::vector<gl_t> pub(d.num_public_inputs + 1);
    caps.resize(4 * ncap * noracles);
    cur.hashes(p.hasher, caps.data(), ncap * noracles);
    const size_t nopen = 2 * (size_t)ncols + 2 * nzs + nq;
    std::vector<gl_t> w(2 * nopen);                    // local, next, zs, zs_next | quotient, with ctl_zs_last between them in the proof
    cur.words(w.data(), w.size() - 2 * nq);
    out.ctl_zs_last.resize(nctl);
    cur.words(out.ctl_zs_last.data(), nctl);
    cur.words(w.data() + w.size() - 2 * nq, 2 * nq);
    const gl2_t* ext = (const gl2_t*)w.data();
    const gl2_t *local = ext, *next = ext + ncols, *zl = ext + 2 * ncols, *zn = zl + nzs, *ql = zn + nzs;
    out.fri = proof_bytes + cur.pos;
    out.fri_len = total - cur.pos - 8 * (size_t)d.num_public_inputs;
    cur.pos += out.fri_len;
    cur.words(pub.data(), d.num_public_inputs);
    // get_challenges (get_challenges.rs:21-59; evm/src/get_challenges.rs:95-149 behind the set's trace caps, CTL challenges and the compact of :39)
    if (ctl) ch.ch.compact();
    else ch.ch.observe_hashes(p.hasher, caps.data(), ncap);
    std::vector<gl_t> sets;
    if (nz) for (uint32_t i = 0; i < 2 * s.q * nc; i++) sets.push_back(ch.ch.challenge());
    if (nzs) ch.ch.observe_hashes(p.hasher, caps.data() + 4 * ncap, ncap);
    gl_t alphas[GL_STARK_MAX_CHALLENGES];
    for (uint32_t j = 0; j < nc; j++) alphas[j] = ch.ch.challenge();
    ch.ch.observe_hashes(p.hasher, caps.data() + 4 * ncap * (noracles - 1), ncap);
    const gl2_t zeta = ch.ch.challenge_ext();
    // FriOpenings order (proof.rs:161-182): [local, zs, quotient], [next, zs_next], [ctl_zs_last lifted]
    std::vector<gl_t>& openings = out.openings;
    openings.clear();
    openings.reserve(2 * nopen + 2 * nctl);
    auto push = [&](const gl2_t* v, size_t k) { for (size_t i = 0; i < k; i++) { openings.push_back(v[i].a); openings.push_back(v[i].b); } };
    push(local, ncols); push(zl, nzs); push(ql, nq); push(next, ncols); push(zn, nzs);
    for (gl_t last : out.ctl_zs_last) { openings.push_back(last); openings.push_back(0); }
    ch.ch.observe_many(openings.data(), openings.size());
    // verifier.rs:81-124: the identity vanishing(zeta) = Z_H(zeta) t(zeta) per challenge
    const gl_t g = gl_host_root_of_unity(p.degree_bits), n_field = gl_t(1) << p.degree_bits, g_inv = gl_canon(gl_inv(g));
    const gl2_t zeta_pow = ext_pow2(zeta, p.degree_bits), z_h = gl2_sub(zeta_pow, gl2_make(1, 0));
    const gl2_t l_first = gl2_mul(z_h, gl2_inv(gl2_scalar(gl2_sub(zeta, gl2_make(1, 0)), n_field)));                      // eval_l_0_and_l_last (verifier.rs:221-228)
    const gl2_t l_last = gl2_mul(z_h, gl2_inv(gl2_scalar(gl2_sub(gl2_scalar(zeta, g), gl2_make(1, 0)), n_field)));
    const gl2_t z_last = gl2_sub(zeta, e_of(g_inv));
    gl2_t accs[GL_STARK_MAX_CHALLENGES];
    vanishing_at(d, s, local, next, pub.data(), alphas, z_last, l_first, l_last, zl, zn, sets.data(), accs, prog, ctl);
    for (uint32_t j = 0; j < nc; j++) {
        gl2_t t = gl2_make(0, 0);                                                                                       // reduce_with_powers(chunk, zeta^n)
        for (uint32_t k = s.q; k-- > 0;) t = gl2_add(gl2_mul(t, zeta_pow), ql[j * s.q + k]);
        const gl2_t lhs = gl2_canon(accs[j]), rhs = gl2_canon(gl2_mul(z_h, t));
        if (lhs.a != rhs.a || lhs.b != rhs.b) return stark_reject(GL_CHECK_VANISHING, check);
    }
    const gl2_t zeta_next = gl2_canon(gl2_scalar(zeta, g));
    out.points[0][0] = zeta.a; out.points[0][1] = zeta.b; out.points[1][0] = zeta_next.a; out.points[1][1] = zeta_next.b; out.points[2][0] = g_inv;
    return GL_OK;
}

int glstark::verify_table(const gl_stark_desc& d, const StarkShape& s, const DagProgram* prog, const gl_fri_params& p, const TableCtl* ctl, const uint8_t* proof_bytes,
                          size_t num_bytes, size_t total, gl_challenger& ch, StarkClaim& claim, uint32_t* check) {
    GL_TRY(stark_host_stage(d, s, prog, p, ctl, proof_bytes, num_bytes, total, ch, claim, check));
    const StarkInstance si(d.num_columns, d.num_challenges, s, nctl_of(ctl), p.degree_bits, gl2_make(claim.points[0][0], claim.points[0][1]));
    return gl_verify_openings(&p, &si.inst, claim.caps.data(), claim.openings.data(), &ch, claim.fri, claim.fri_len, check);
}

// gl_stark_verify and gl_stark_dag_verify
int glstark::stark_verify(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check) {
    StarkShape s;
    DagProgram prog;
    GL_TRY(stark_check(desc, params, &s, false, dag, &prog));
    StarkClaim claim;
    gl_challenger ch{glhost::HostChallenger(params->hasher)};
    const size_t total = table_proof_bytes(*params, desc->num_columns, desc->num_public_inputs, desc->num_challenges, s, 0);
    return verify_table(*desc, s, dag ? &prog : nullptr, *params, nullptr, proof_bytes, num_bytes, total, ch, claim, check);
}

// ---- verify_stark_proof for many proofs of one Stark: the host stage per proof on host threads, each proof's FriProof a claim of the
// device batch verifier for the STARK's instance (openings_verify.hip) ----
struct gl_stark_batch_verifier {
    gl_openings_batch_verifier* inner = nullptr;
    gl_fri_params params;
    StarkShape shape;
    gl_stark_desc desc;                                // its tables point into the vectors below: the caller's may go away
    std::vector<uint32_t> filter, num_terms, term_nf, factors, pair_len, pair_columns;
    std::vector<uint64_t> coeff;
    bool dag = false;
    DagProgram prog;                                   // compiled once
    struct Lane { StarkClaim claim; gl_challenger ch{glhost::HostChallenger(GL_HASHER_POSEIDON)}; };
    std::vector<Lane> lanes;                           // one per host thread
    size_t proof_bytes = 0;
};

extern "C" void gl_stark_batch_verifier_free(gl_stark_batch_verifier* v) noexcept {
    if (!v) return;
    gl_openings_batch_verifier_free(v->inner);
    delete v;
}

extern "C" int gl_stark_batch_verifier_new(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, uint32_t max_batch,
                                           uint32_t host_threads, gl_stark_batch_verifier** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_stark_batch_verifier_new: null argument");
    *out = nullptr;
    GL_REQUIRE(ctx && desc && params, GL_ERR_ARG, "gl_stark_batch_verifier_new: null argument");
    std::unique_ptr<gl_stark_batch_verifier, void (*)(gl_stark_batch_verifier*)> v(new gl_stark_batch_verifier(), gl_stark_batch_verifier_free);
    GL_TRY(stark_check(desc, params, &v->shape, true, dag, &v->prog));            // gl_stark_check (gl_stark_dag_check) itself: reductions by 16 only
    const StarkShape& s = v->shape;
    const gl_stark_desc& d = *desc;
    v->params = *params; v->dag = dag != nullptr; v->desc = d;
    auto keep = [](auto& vec, const auto* from, size_t k) { if (from && k) vec.assign(from, from + k); return vec.empty() ? decltype(vec.data())(nullptr) : vec.data(); };
    v->desc.constraint_filter = keep(v->filter, d.constraint_filter, d.num_constraints);
    v->desc.constraint_num_terms = keep(v->num_terms, d.constraint_num_terms, d.num_constraints);
    v->desc.term_coeff = keep(v->coeff, d.term_coeff, s.terms);
    v->desc.term_num_factors = keep(v->term_nf, d.term_num_factors, s.terms);
    v->desc.factors = keep(v->factors, d.factors, s.factors);
    v->desc.pair_len = keep(v->pair_len, d.pair_len, d.num_permutation_pairs);
    v->desc.pair_columns = keep(v->pair_columns, d.pair_columns, 2 * s.column_pairs);
    const StarkInstance si(d.num_columns, d.num_challenges, s, 0, params->degree_bits);
    GL_TRY(glopen::batch_new(ctx, params, &si.inst, max_batch, host_threads, &v->inner));
    v->lanes.resize(host_threads ? host_threads : 1);
    v->proof_bytes = table_proof_bytes(*params, d.num_columns, d.num_public_inputs, d.num_challenges, s, 0);
    *out = v.release();
    return GL_OK;
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_batch_verifier_verify(gl_stark_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count, int32_t* verdicts,
                                              uint32_t* checks) try {
    GL_REQUIRE(v, GL_ERR_ARG, "gl_stark_batch_verifier_verify: null verifier");
    if (!count) return GL_OK;
    GL_REQUIRE(proofs && num_bytes && verdicts, GL_ERR_ARG, "gl_stark_batch_verifier_verify: null argument");
    return glopen::batch_verify(v->inner, count, [&](size_t lane, size_t i, gl_openings_claim& claim, uint32_t* check) -> int {
        GL_REQUIRE(proofs[i], GL_ERR_ARG, "gl_stark_batch_verifier_verify: null proof");
        StarkClaim& c = v->lanes[lane].claim;
        gl_challenger& ch = v->lanes[lane].ch;
        ch.ch = glhost::HostChallenger(v->params.hasher);
        GL_TRY(stark_host_stage(v->desc, v->shape, v->dag ? &v->prog : nullptr, v->params, nullptr, proofs[i], num_bytes[i], v->proof_bytes, ch, c, check));
        claim.caps = c.caps.data(); claim.openings = c.openings.data(); claim.points = c.points; claim.challenger = &ch;
        claim.proof = c.fri; claim.num_bytes = c.fri_len;
        return GL_OK;
    }, verdicts, checks);
} catch (...) { return gl_caught(); }

// the launches of k_stark_seg_products and k_stark_seg_scan for the other running products (stark_set.hip): d_seg[nz][nseg] becomes the
// exclusive prefix of the segment products of d_fac[nz][n]
void glstark::seg_products_scan(hipStream_t st, const gl_t* d_fac, uint32_t n, uint32_t nz, gl_t* d_seg) {
    const uint32_t nseg = (n + GLS_SEG - 1) / GLS_SEG;
    hipLaunchKernelGGL(k_stark_seg_products, dim3(nseg, nz), dim3(256), 0, st, d_fac, n, d_seg);
    hipLaunchKernelGGL(k_stark_seg_scan, dim3((nz + 63) / 64), dim3(64), 0, st, d_seg, nseg, nz);
}
