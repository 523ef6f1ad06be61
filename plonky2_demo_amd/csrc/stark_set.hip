// STARK table sets (evm/src/cross_table_lookup.rs, evm/src/stark.rs:83-142): tables as gl_stark_desc tied by cross-table lookups handed
// over as data -- gl_stark_set_desc -- its validation, the CTL running products Z and the CTL checks of the quotient and of the verifier.
// Per table everything else is stark.hip's code: its prover body and verification stage take the table's TableCtl from here.
#include "stark_internal.hpp"
#include "proof.hpp"
#include "stark_ctl_kernels.cuh"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

using namespace glstark;

struct CtlZ { uint32_t twc, chal; };            // one CTL Z of a table: its TableWithColumns and its challenge
struct glstark::SetShape {
    uint32_t num_tables = 0, nc = 0;
    std::vector<StarkShape> shapes;             // per table
    std::vector<std::vector<CtlZ>> ctl_zs;      // per table, in cross_table_lookup_data's order
    std::vector<uint32_t> col_off;              // [Columns + 1] start of each Column's terms
    std::vector<uint32_t> twc_col0;             // [twcs] first Column of each TableWithColumns
    std::vector<DagProgram> progs;              // per table: its compiled DAG where dags[t] is given (gl_stark_set_dag_*)
};

namespace {

// dags: null, or [num_tables] with a null entry for a table in term-list form
int stark_set_check(const gl_stark_set_desc* desc, SetShape* shape, bool prover = true, const gl_stark_dag* const* dags = nullptr) {
    GL_REQUIRE(desc, GL_ERR_ARG, "gl_stark_set: null description");
    const gl_stark_set_desc& d = *desc;
    GL_REQUIRE(d.num_tables >= 1 && d.num_tables <= GL_STARK_SET_MAX_TABLES, GL_ERR_ARG, "gl_stark_set: 1..8 tables");
    GL_REQUIRE(d.tables && d.params, GL_ERR_ARG, "gl_stark_set: null tables / params");
    SetShape s;
    s.num_tables = d.num_tables; s.nc = d.tables[0].num_challenges;
    s.shapes.resize(d.num_tables); s.ctl_zs.resize(d.num_tables); s.progs.resize(d.num_tables);
    for (uint32_t t = 0; t < d.num_tables; t++) GL_TRY(stark_check(&d.tables[t], &d.params[t], &s.shapes[t], prover, dags ? dags[t] : nullptr, &s.progs[t]));
    // one StarkConfig for the set (evm/src/config.rs): only degree_bits, and with it the number of reductions, is a table's own
    const gl_fri_params& p0 = d.params[0];
    uint32_t arity = 0;
    for (uint32_t t = 0; t < d.num_tables; t++) {
        const gl_fri_params& p = d.params[t];
        GL_REQUIRE(p.hasher == p0.hasher && p.rate_bits == p0.rate_bits && p.cap_height == p0.cap_height && p.num_query_rounds == p0.num_query_rounds &&
                   p.proof_of_work_bits == p0.proof_of_work_bits && d.tables[t].num_challenges == s.nc, GL_ERR_ARG,
                   "gl_stark_set: hasher, rate_bits, cap_height, query rounds, proof-of-work bits and num_challenges must agree across the tables");
        for (uint32_t r = 0; r < p.num_fri_rounds; r++) {
            if (!arity) arity = p.fri_arity_bits[r];
            GL_REQUIRE(p.fri_arity_bits[r] == arity, GL_ERR_ARG, "gl_stark_set: the tables' reductions must have one arity (one reduction strategy across the tables)");
        }
    }
    // the three pools, consumed in order
    GL_REQUIRE(d.num_lookups <= GL_CTL_MAX_LOOKUPS, GL_ERR_ARG, "gl_stark_set: at most 32 cross-table lookups");
    GL_REQUIRE(!d.num_lookups || (d.lookup_num_looking && d.twc_table && d.twc_num_columns && d.twc_has_filter && d.column_num_terms && d.column_constant),
               GL_ERR_ARG, "gl_stark_set: null lookup table");
    GL_REQUIRE(d.num_twcs <= GL_CTL_MAX_LOOKUPS * (GL_CTL_MAX_LOOKING + 1) && d.num_ctl_columns <= GL_CTL_MAX_LOOKUPS * (GL_CTL_MAX_LOOKING + 1) * (GL_CTL_MAX_COLUMNS + 1),
               GL_ERR_ARG, "gl_stark_set: more TableWithColumns / Columns than 32 lookups can use");
    s.col_off.assign(1, 0);
    uint32_t twc = 0, col = 0;
    std::vector<uint8_t> seen;
    for (uint32_t l = 0; l < d.num_lookups; l++) {
        const uint32_t looking = d.lookup_num_looking[l];
        GL_REQUIRE(looking >= 1 && looking <= GL_CTL_MAX_LOOKING, GL_ERR_ARG, "gl_stark_set: a lookup has 1..8 looking tables");
        GL_REQUIRE(looking + 1 <= d.num_twcs - twc, GL_ERR_ARG, "gl_stark_set: the lookups list more TableWithColumns than the pool holds");
        const uint32_t first = twc;
        for (uint32_t k = 0; k <= looking; k++, twc++) {
            const uint32_t table = d.twc_table[twc], ncols = d.twc_num_columns[twc], has_filter = d.twc_has_filter[twc];
            GL_REQUIRE(table < d.num_tables, GL_ERR_ARG, "gl_stark_set: table index out of range");
            GL_REQUIRE(ncols >= 1 && ncols <= GL_CTL_MAX_COLUMNS, GL_ERR_ARG, "gl_stark_set: a TableWithColumns has 1..16 columns");
            GL_REQUIRE(has_filter <= 1, GL_ERR_ARG, "gl_stark_set: twc_has_filter is 0 or 1");
            GL_REQUIRE(ncols == d.twc_num_columns[first], GL_ERR_ARG, "gl_stark_set: the tables of a lookup differ in their number of columns");
            GL_REQUIRE(ncols + has_filter <= d.num_ctl_columns - col, GL_ERR_ARG, "gl_stark_set: the lookups list more Columns than the pool holds");
            // Z(g x) - Z(x) (f c + 1 - f) has three trace-degree factors under a filter: its quotient needs q >= 2
            GL_REQUIRE(!has_filter || s.shapes[table].q >= 2, GL_ERR_ARG, "gl_stark_set: a filtered lookup needs constraint_degree >= 3 on its table");
            s.twc_col0.push_back(col);
            for (uint32_t c = 0; c < ncols + has_filter; c++, col++) {
                const uint32_t nt = d.column_num_terms[col], off = s.col_off.back();
                GL_REQUIRE(nt <= GL_CTL_MAX_TERMS, GL_ERR_ARG, "gl_stark_set: a Column has more than 64 terms");
                GL_REQUIRE(!nt || (d.term_column && d.term_coeff), GL_ERR_ARG, "gl_stark_set: null Column term table");
                seen.assign(d.tables[table].num_columns, 0);
                for (uint32_t k2 = 0; k2 < nt; k2++) {
                    const uint32_t tc = d.term_column[off + k2];
                    GL_REQUIRE(tc < d.tables[table].num_columns, GL_ERR_ARG, "gl_stark_set: a Column's trace column is out of range");
                    GL_REQUIRE(!seen[tc], GL_ERR_ARG, "gl_stark_set: duplicate columns in a Column");
                    seen[tc] = 1;
                }
                s.col_off.push_back(off + nt);
            }
        }
        // cross_table_lookup_data's order (cross_table_lookup.rs:232-274): challenge by challenge, looking tables, then the looked one
        for (uint32_t chal = 0; chal < s.nc; chal++)
            for (uint32_t k = 0; k <= looking; k++) s.ctl_zs[d.twc_table[first + k]].push_back(CtlZ{first + k, chal});
    }
    GL_REQUIRE(twc == d.num_twcs && col == d.num_ctl_columns, GL_ERR_ARG, "gl_stark_set: the lookups do not consume the TableWithColumns / Column pools exactly");
    for (uint32_t t = 0; t < d.num_tables; t++) {
        GL_REQUIRE(s.shapes[t].nz || !s.ctl_zs[t].empty(), GL_ERR_ARG, "gl_stark_set: a table with neither permutation pairs nor a cross-table lookup (No CTL?)");
        const StarkInstance si(d.tables[t].num_columns, s.nc, s.shapes[t], (uint32_t)s.ctl_zs[t].size(), d.params[t].degree_bits);
        GL_TRY(glfri::check(&d.params[t], &si.inst, prover));
    }
    if (shape) *shape = std::move(s);
    return GL_OK;
}

}  // namespace

struct gl_stark_set {
    gl_ctx* ctx = nullptr;
    uint32_t num_tables = 0, nc = 0;
    size_t proof_bytes = 0;                                 // the tables' table_proof_bytes, CTL Zs counted
    gl_stark* tables[GL_STARK_SET_MAX_TABLES] = {nullptr};
    uint32_t nctl[GL_STARK_SET_MAX_TABLES] = {0};
    void* d_prog[GL_STARK_SET_MAX_TABLES] = {nullptr};      // per table one block: the CTL program of its Zs
    GlStarkCtl prog[GL_STARK_SET_MAX_TABLES];               // pointers into d_prog (trace, ch and n are the call's)
};

extern "C" int gl_stark_set_check(const gl_stark_set_desc* desc) try {
    return stark_set_check(desc, nullptr);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_dag_check(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags) try {
    return stark_set_check(desc, nullptr, true, dags);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_num_zs(const gl_stark_set_desc* desc, uint32_t table, uint32_t* num_permutation_zs, uint32_t* num_ctl_zs) try {
    SetShape sh;
    GL_TRY(stark_set_check(desc, &sh, false));
    GL_REQUIRE(table < sh.num_tables, GL_ERR_ARG, "gl_stark_set_num_zs: table index out of range");
    if (num_permutation_zs) *num_permutation_zs = sh.shapes[table].nz;
    if (num_ctl_zs) *num_ctl_zs = (uint32_t)sh.ctl_zs[table].size();
    return GL_OK;
} catch (...) { return gl_caught(); }

extern "C" void gl_stark_set_free(gl_stark_set* s) noexcept {
    if (!s) return;
    for (uint32_t t = 0; t < GL_STARK_SET_MAX_TABLES; t++) {
        if (s->ctx && s->d_prog[t]) s->ctx->pool_release(s->d_prog[t]);
        gl_stark_free(s->tables[t]);
    }
    if (s->ctx) gl_ctx_release(s->ctx);
    delete s;
}

namespace {
int set_create(gl_ctx* ctx, const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, gl_stark_set** out);
int set_verify(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check, uint32_t* table);
}  // namespace

extern "C" int gl_stark_set_create(gl_ctx* ctx, const gl_stark_set_desc* desc, gl_stark_set** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_stark_set_create: null out");
    *out = nullptr;
    return set_create(ctx, desc, nullptr, out);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_dag_create(gl_ctx* ctx, const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, gl_stark_set** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_stark_set_dag_create: null out");
    *out = nullptr;
    return set_create(ctx, desc, dags, out);
} catch (...) { return gl_caught(); }

namespace {

int set_create(gl_ctx* ctx, const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, gl_stark_set** out) {
    GL_REQUIRE(ctx, GL_ERR_ARG, "gl_stark_set_create: null context");
    SetShape sh;
    GL_TRY(stark_set_check(desc, &sh, true, dags));
    GL_TRY(ctx->activate());
    const gl_stark_set_desc& d = *desc;
    std::unique_ptr<gl_stark_set, void (*)(gl_stark_set*)> s(new gl_stark_set(), gl_stark_set_free);
    s->ctx = ctx; ctx->retain();
    s->num_tables = d.num_tables; s->nc = sh.nc;
    for (uint32_t t = 0; t < d.num_tables; t++) {
        GL_TRY(stark_create(ctx, &d.tables[t], dags ? dags[t] : nullptr, &d.params[t], &s->tables[t]));
        const std::vector<CtlZ>& zs = sh.ctl_zs[t];
        s->nctl[t] = (uint32_t)zs.size();
        s->proof_bytes += table_proof_bytes(d.params[t], d.tables[t].num_columns, d.tables[t].num_public_inputs, sh.nc, sh.shapes[t], s->nctl[t]);
        ::memset((void*)&s->prog[t], 0, sizeof s->prog[t]);
        if (zs.empty()) continue;
        // the table's own image of the Columns its Zs use, 8-byte words first: [coeff | const] then [z_prog | col_off | term_col]
        std::vector<gl_t> coeff, cst;
        std::vector<uint32_t> z_prog, col_off(1, 0), term_col;
        for (const CtlZ& z : zs) {
            const uint32_t ncols = d.twc_num_columns[z.twc], has_filter = d.twc_has_filter[z.twc];
            z_prog.push_back((uint32_t)cst.size()); z_prog.push_back(ncols); z_prog.push_back(has_filter); z_prog.push_back(z.chal);
            for (uint32_t c = sh.twc_col0[z.twc]; c < sh.twc_col0[z.twc] + ncols + has_filter; c++) {
                cst.push_back(gl_canon(d.column_constant[c]));
                for (uint32_t k = sh.col_off[c]; k < sh.col_off[c + 1]; k++) { term_col.push_back(d.term_column[k]); coeff.push_back(gl_canon(d.term_coeff[k])); }
                col_off.push_back((uint32_t)term_col.size());
            }
        }
        const size_t nterms = coeff.size(), ncolumns = cst.size();
        std::vector<gl_t> words(coeff);
        words.insert(words.end(), cst.begin(), cst.end());
        std::vector<uint32_t> u32(z_prog);
        u32.insert(u32.end(), col_off.begin(), col_off.end());
        u32.insert(u32.end(), term_col.begin(), term_col.end());
        u32.resize(u32.size() + 2);
        const size_t bytes64 = words.size() * sizeof(gl_t), bytes32 = u32.size() * sizeof(uint32_t);
        GL_TRY(ctx->pool_alloc(bytes64 + bytes32, &s->d_prog[t]));
        GL_TRY(gl_copy_h2d(ctx, s->d_prog[t], words.data(), bytes64));
        GL_TRY(gl_copy_h2d(ctx, (char*)s->d_prog[t] + bytes64, u32.data(), bytes32));
        GlStarkCtl& g = s->prog[t];
        g.term_coeff = (const gl_t*)s->d_prog[t]; g.col_const = g.term_coeff + nterms;
        g.z_prog = (const uint32_t*)((const char*)s->d_prog[t] + bytes64); g.col_off = g.z_prog + z_prog.size(); g.term_col = g.col_off + ncolumns + 1;
    }
    *out = s.release();
    return GL_OK;
}

int check_set_args(gl_ctx* ctx, const gl_stark_set* s, uint32_t table) {
    GL_REQUIRE(ctx && s, GL_ERR_ARG, "gl_stark_set: null context / set");
    GL_REQUIRE(s->ctx == ctx, GL_ERR_ARG, "gl_stark_set: the set was created on another context");
    GL_REQUIRE(table < s->num_tables, GL_ERR_ARG, "gl_stark_set: table index out of range");
    return ctx->activate();
}

// the prover's view of a table of the set
TableCtl ctl_of(const gl_stark_set* s, uint32_t table, const uint64_t* ctl_challenges) {
    TableCtl c;
    c.table = table; c.nctl = s->nctl[table]; c.challenges = ctl_challenges; c.set = s;
    return c;
}
// the set's challenges [num_challenges][2], canonical, into a pool block
int upload_ctl_challenges(gl_ctx* ctx, const TableCtl& ctl, DevBuf& d_ch) {
    std::vector<gl_t> ch(2 * (size_t)ctl.set->nc);
    for (size_t i = 0; i < ch.size(); i++) ch[i] = gl_canon(ctl.challenges[i]);
    GL_TRY(d_ch.alloc(ch.size() * sizeof(gl_t)));
    return gl_copy_h2d(ctx, d_ch.p, ch.data(), ch.size() * sizeof(gl_t));
}

}  // namespace

// partial_products (cross_table_lookup.rs:279-306) of every CTL Z of a table
int glstark::ctl_z_values(gl_ctx* ctx, const TableCtl& ctl, const gl_t* d_trace, gl_t* d_z) {
    const gl_stark_set* s = ctl.set;
    const uint32_t table = ctl.table, n = (uint32_t)s->tables[table]->n, nzc = ctl.nctl, nseg = (n + GLS_SEG - 1) / GLS_SEG;
    hipStream_t stream = ctx->stream;
    DevBuf d_ch(ctx), d_fac(ctx), d_seg(ctx), d_flag(ctx);
    GL_TRY(upload_ctl_challenges(ctx, ctl, d_ch));
    GL_TRY(d_fac.alloc((size_t)nzc * n * sizeof(gl_t)));
    GL_TRY(d_seg.alloc((size_t)nzc * nseg * sizeof(gl_t)));
    GL_TRY(d_flag.alloc(sizeof(uint32_t)));
    GL_CHECK_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), stream));
    GlStarkCtl p = s->prog[table];
    p.trace = d_trace; p.ch = d_ch.as<const gl_t>(); p.n = n;
    ctx->timing_begin("compute CTL Z polys");
    hipLaunchKernelGGL(k_stark_ctl_factors, dim3(nseg, nzc), dim3(256), 0, stream, p, d_fac.as<gl_t>(), d_flag.as<uint32_t>());
    seg_products_scan(stream, d_fac.as<const gl_t>(), n, nzc, d_seg.as<gl_t>());
    hipLaunchKernelGGL(k_stark_z_finalize_inclusive, dim3(nseg, nzc), dim3(256), 0, stream, d_fac.as<const gl_t>(), d_seg.as<const gl_t>(), n, d_z);
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    uint32_t flag = 0;
    GL_TRY(read_flag(ctx, d_flag.as<uint32_t>(), &flag));
    GL_REQUIRE(!flag, GL_ERR_ARG, "gl_stark_set: non-binary CTL filter (a filter Column takes a value other than 0 and 1 on some row)");
    return GL_OK;
}

extern "C" int gl_stark_set_ctl_z_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* ctl_challenges,
                                         uint64_t* h_out) try {
    GL_TRY(check_set_args(ctx, s, table));
    GL_REQUIRE(d_trace_values && ctl_challenges && h_out, GL_ERR_ARG, "gl_stark_set_ctl_z_values: null argument");
    GL_REQUIRE(s->nctl[table], GL_ERR_ARG, "gl_stark_set_ctl_z_values: the table stands in no cross-table lookup");
    const size_t bytes = (size_t)s->nctl[table] * s->tables[table]->n * sizeof(gl_t);
    DevBuf d_z(ctx);
    GL_TRY(d_z.alloc(bytes));
    GL_TRY(ctl_z_values(ctx, ctl_of(s, table, ctl_challenges), d_trace_values, d_z.as<gl_t>()));
    return gl_copy_d2h(ctx, h_out, d_z.p, bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_zs(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* permutation_challenges,
                               const uint64_t* ctl_challenges, gl_batch** zs) try {
    GL_REQUIRE(zs, GL_ERR_ARG, "gl_stark_set_zs: null out");
    *zs = nullptr;
    GL_TRY(check_set_args(ctx, s, table));
    GL_REQUIRE(d_trace_values && (ctl_challenges || !s->nctl[table]), GL_ERR_ARG, "gl_stark_set_zs: null argument");
    GL_REQUIRE((s->tables[table]->s.nz != 0) == (permutation_challenges != nullptr), GL_ERR_ARG,
               "gl_stark_set_zs: the permutation challenge sets go with permutation pairs (null without)");
    const TableCtl ctl = ctl_of(s, table, ctl_challenges);
    return zs_commit(ctx, s->tables[table], &ctl, d_trace_values, permutation_challenges, zs);
} catch (...) { return gl_caught(); }

// the CTL pass of the quotient: k_stark_quotient_ctl folds the table's CTL checks into d_q behind k_stark_quotient's
int glstark::ctl_quotient_pass(gl_ctx* ctx, const TableCtl& ctl, const gl_batch* trace, const gl_batch* zs, const uint64_t* alphas, DevBuf& d_q) {
    const gl_stark_set* s = ctl.set;
    const gl_stark* st = s->tables[ctl.table];
    const uint32_t nctl = ctl.nctl;
    DevBuf d_ch(ctx);
    GL_TRY(upload_ctl_challenges(ctx, ctl, d_ch));
    GlStarkQuotCtl q;
    ::memset((void*)&q, 0, sizeof q);
    q.c = s->prog[ctl.table];
    q.c.trace = trace->lde; q.c.ch = d_ch.as<const gl_t>(); q.c.n = 0;
    q.stride = trace->N(); q.zs = zs->lde + (size_t)st->s.nz * q.stride;
    q.xpow_lo = st->xt.lo; q.xpow_hi = st->xt.hi; q.lfirst = st->d_lagrange; q.out = d_q.as<gl_t>();
    for (uint32_t j = 0; j < s->nc; j++) { q.alphas[j] = gl_canon(alphas[j]); q.alpha_pow[j] = gl_canon(gl_exp(q.alphas[j], 2 * (uint64_t)nctl)); }
    for (int i = 0; i < 8; i++) q.zh_inv[i] = st->zh_inv[i];
    q.last = st->last;
    q.size = (uint32_t)st->size; q.step = 1u << (st->params.rate_bits - st->s.qdb); q.next_step = 1u << st->s.qdb; q.nctl = nctl;
    const dim3 grid((unsigned)((st->size + 255) / 256)), block(256);
    ctx->timing_begin("compute quotient polys (CTL checks)");
    switch (s->nc) {
        case 1: hipLaunchKernelGGL(k_stark_quotient_ctl<1>, grid, block, 0, ctx->stream, q); break;
        case 2: hipLaunchKernelGGL(k_stark_quotient_ctl<2>, grid, block, 0, ctx->stream, q); break;
        case 3: hipLaunchKernelGGL(k_stark_quotient_ctl<3>, grid, block, 0, ctx->stream, q); break;
        default: hipLaunchKernelGGL(k_stark_quotient_ctl<4>, grid, block, 0, ctx->stream, q); break;
    }
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}

namespace {

// the set's quotient entries: their argument checks in front of the per-table quotient phase
int set_quotient_phase(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs, const uint64_t* permutation_challenges,
                       const uint64_t* ctl_challenges, const uint64_t* alphas, const uint64_t* public_inputs, DevBuf& d_q) {
    GL_TRY(check_set_args(ctx, s, table));
    const gl_stark* st = s->tables[table];
    const uint32_t nz = st->s.nz, nctl = s->nctl[table];
    GL_REQUIRE(zs && (ctl_challenges || !nctl), GL_ERR_ARG, "gl_stark_set quotient: null Z batch / CTL challenges");
    GL_REQUIRE((nz != 0) == (permutation_challenges != nullptr), GL_ERR_ARG, "gl_stark_set quotient: the permutation challenge sets go with permutation pairs (null without)");
    GL_TRY(check_stark_batch(st, zs, nz + nctl, "gl_stark_set quotient: the Z batch does not match the description / params (permutation Zs, then CTL Zs)"));
    const TableCtl ctl = ctl_of(s, table, ctl_challenges);
    return quotient_phase(ctx, st, trace, zs, permutation_challenges, alphas, public_inputs, d_q, &ctl);
}

}  // namespace

extern "C" int gl_stark_set_quotient_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs,
                                            const uint64_t* permutation_challenges, const uint64_t* ctl_challenges, const uint64_t* alphas,
                                            const uint64_t* public_inputs, uint64_t* h_out) try {
    GL_REQUIRE(h_out, GL_ERR_ARG, "gl_stark_set_quotient_values: null out");
    DevBuf d_q(ctx);
    GL_TRY(set_quotient_phase(ctx, s, table, trace, zs, permutation_challenges, ctl_challenges, alphas, public_inputs, d_q));
    return gl_copy_d2h(ctx, h_out, d_q.p, (size_t)s->nc * s->tables[table]->size * sizeof(gl_t));
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_quotient_polys(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs,
                                           const uint64_t* permutation_challenges, const uint64_t* ctl_challenges, const uint64_t* alphas,
                                           const uint64_t* public_inputs, gl_batch** quotient) try {
    GL_REQUIRE(quotient, GL_ERR_ARG, "gl_stark_set_quotient_polys: null out");
    *quotient = nullptr;
    DevBuf d_q(ctx);
    GL_TRY(set_quotient_phase(ctx, s, table, trace, zs, permutation_challenges, ctl_challenges, alphas, public_inputs, d_q));
    return quotient_commit(ctx, s->tables[table], d_q, quotient);
} catch (...) { return gl_caught(); }

// ---- the whole set prover and the verifier (evm/src/prover.rs:94-467, verifier.rs:29-216, cross_table_lookup.rs:542-569) ------------------
namespace {

int set_prove_device(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* d_cols, const uint64_t* const* h_public_inputs, uint8_t* h_out, size_t cap_bytes,
                     size_t* num_bytes) {
    GL_TRY(check_set_args(ctx, s, 0));
    GL_REQUIRE(d_cols && num_bytes, GL_ERR_ARG, "gl_stark_set_prove: null argument");
    const size_t total = s->proof_bytes;
    *num_bytes = total;
    GL_REQUIRE(h_out && cap_bytes >= total, GL_ERR_ARG, "gl_stark_set_prove: output too small (gl_stark_set_proof_size)");
    const gl_fri_params& p0 = s->tables[0]->params;
    const size_t ncap = size_t(1) << p0.cap_height;
    gl_challenger ch{glhost::HostChallenger(p0.hasher)};
    // every trace committed, every cap observed in table order (prover.rs:114-146)
    BatchHolder traces[GL_STARK_SET_MAX_TABLES];
    std::vector<gl_t> caps(4 * ncap * s->num_tables);
    for (uint32_t t = 0; t < s->num_tables; t++) {
        const gl_stark* st = s->tables[t];
        GL_REQUIRE(d_cols[t], GL_ERR_ARG, "gl_stark_set_prove: null trace");
        GL_TRY(gl_batch_from_device_h(ctx, p0.hasher, d_cols[t], st->num_columns, st->n, p0.rate_bits, p0.cap_height, 1, &traces[t].b));
        GL_TRY(gl_batch_cap(traces[t].b, caps.data() + 4 * ncap * t));
    }
    for (uint32_t t = 0; t < s->num_tables; t++) ch.ch.observe_hashes(p0.hasher, caps.data() + 4 * ncap * t, ncap);
    gl_t ctl_ch[2 * GL_STARK_MAX_CHALLENGES];
    for (uint32_t i = 0; i < 2 * s->nc; i++) ctl_ch[i] = ch.ch.challenge();         // get_grand_product_challenge_set: beta, gamma per challenge
    std::vector<uint8_t> o;
    o.reserve(total);
    // prove_single_table (evm/src/prover.rs:288-467): the trace cap, the compact, then the table's body (stark.hip)
    for (uint32_t t = 0; t < s->num_tables; t++) {
        const uint64_t* pis = h_public_inputs ? h_public_inputs[t] : nullptr;
        GL_REQUIRE(pis || !s->tables[t]->num_public_inputs, GL_ERR_ARG, "gl_stark_set_prove: null public inputs of a table that has some");
        put_hashes(o, p0.hasher, caps.data() + 4 * ncap * t, ncap);
        ch.ch.compact();
        const TableCtl ctl = ctl_of(s, t, ctl_ch);
        GL_TRY(prove_table(ctx, s->tables[t], &ctl, d_cols[t], traces[t].b, pis, ch, o, "gl_stark_set_prove"));
    }
    GL_REQUIRE(o.size() == total, GL_ERR_INTERNAL, "gl_stark_set_prove: the proof has another size than gl_stark_set_proof_size");
    ::memcpy(h_out, o.data(), total);
    return GL_OK;
}

}  // namespace

extern "C" size_t gl_stark_set_proof_size(const gl_stark_set* s) noexcept { return s ? s->proof_bytes : 0; }

extern "C" int gl_stark_set_prove_device(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* d_cols, const uint64_t* const* h_public_inputs,
                                         uint8_t* h_out, size_t cap_bytes, size_t* num_bytes) try {
    return set_prove_device(ctx, s, d_cols, h_public_inputs, h_out, cap_bytes, num_bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_prove(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* const* h_trace_cols, const uint64_t* const* h_public_inputs,
                                  uint8_t* h_out, size_t cap_bytes, size_t* num_bytes) try {
    GL_TRY(check_set_args(ctx, s, 0));
    GL_REQUIRE(h_trace_cols, GL_ERR_ARG, "gl_stark_set_prove: null traces");
    std::vector<DevBuf> d_cols;
    d_cols.reserve(s->num_tables);
    const uint64_t* ptrs[GL_STARK_SET_MAX_TABLES] = {nullptr};
    for (uint32_t t = 0; t < s->num_tables; t++) {
        const gl_stark* st = s->tables[t];
        GL_REQUIRE(h_trace_cols[t], GL_ERR_ARG, "gl_stark_set_prove: null trace");
        d_cols.emplace_back(ctx);
        GL_TRY(d_cols.back().alloc((size_t)st->num_columns * st->n * sizeof(gl_t)));
        for (uint32_t c = 0; c < st->num_columns; c++) {
            GL_REQUIRE(h_trace_cols[t][c], GL_ERR_ARG, "gl_stark_set_prove: null trace column");
            GL_CHECK_HIP(hipMemcpyAsync(d_cols.back().as<gl_t>() + (size_t)c * st->n, h_trace_cols[t][c], st->n * sizeof(gl_t), hipMemcpyHostToDevice, ctx->stream));
        }
        ptrs[t] = d_cols.back().as<uint64_t>();
    }
    GL_CHECK_HIP(gl_stream_wait(ctx->stream));          // pageable sources must not be reused before the copies land
    return set_prove_device(ctx, s, ptrs, h_public_inputs, h_out, cap_bytes, num_bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_verify(const gl_stark_set_desc* desc, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check, uint32_t* table) try {
    if (check) *check = GL_CHECK_ACCEPTED;
    return set_verify(desc, nullptr, proof_bytes, num_bytes, check, table);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_dag_verify(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check,
                                       uint32_t* table) try {
    if (check) *check = GL_CHECK_ACCEPTED;
    return set_verify(desc, dags, proof_bytes, num_bytes, check, table);
} catch (...) { return gl_caught(); }

// eval_cross_table_lookup_checks (CtlCheckVars::from_proofs, cross_table_lookup.rs:325-414)
void glstark::ctl_checks_at(const TableCtl& ctl, const gl2_t* local, const gl2_t* next, const gl2_t* zs, const gl2_t* zs_next, gl2_t l_first, gl2_t z_last,
                            const std::function<void(gl2_t)>& consume) {
    const gl_stark_set_desc& d = *ctl.desc;
    const SetShape& sh = *ctl.shape;
    for (uint32_t k = 0; k < ctl.nctl; k++) {
        const CtlZ& z = sh.ctl_zs[ctl.table][k];
        const uint32_t c0 = sh.twc_col0[z.twc], nco = d.twc_num_columns[z.twc], has_filter = d.twc_has_filter[z.twc];
        const gl_t beta = gl_canon(ctl.challenges[2 * z.chal]), gamma = gl_canon(ctl.challenges[2 * z.chal + 1]);
        auto column = [&](uint32_t c, const gl2_t* v) {
            gl2_t acc = e_of(d.column_constant[c]);
            for (uint32_t x = sh.col_off[c]; x < sh.col_off[c + 1]; x++) acc = gl2_add(acc, gl2_scalar(v[d.term_column[x]], gl_canon(d.term_coeff[x])));
            return acc;
        };
        auto selected = [&](const gl2_t* v) {
            gl2_t comb = gl2_make(0, 0);
            for (uint32_t c = nco; c-- > 0;) comb = gl2_add(gl2_scalar(comb, beta), column(c0 + c, v));
            comb = gl2_add(comb, e_of(gamma));
            if (!has_filter) return comb;
            const gl2_t f = column(c0 + nco, v);
            return gl2_sub(gl2_add(gl2_mul(f, comb), gl2_make(1, 0)), f);           // select(f, x) = f x + 1 - f
        };
        consume(gl2_mul(gl2_sub(zs[k], selected(local)), l_first));
        consume(gl2_mul(gl2_sub(zs_next[k], gl2_mul(zs[k], selected(next))), z_last));
    }
}

namespace {

int set_verify(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check, uint32_t* table) {
    SetShape sh;
    GL_TRY(stark_set_check(desc, &sh, false, dags));
    GL_REQUIRE(proof_bytes || !num_bytes, GL_ERR_ARG, "gl_stark_set_verify: null proof");
    const gl_stark_set_desc& d = *desc;
    const uint32_t T = d.num_tables, nc = sh.nc;
    if (table) *table = T;
    const gl_fri_params& p0 = d.params[0];
    const size_t ncap = size_t(1) << p0.cap_height;
    size_t offs[GL_STARK_SET_MAX_TABLES + 1] = {0};
    for (uint32_t t = 0; t < T; t++)
        offs[t + 1] = offs[t] + table_proof_bytes(d.params[t], d.tables[t].num_columns, d.tables[t].num_public_inputs, nc, sh.shapes[t], (uint32_t)sh.ctl_zs[t].size());
    if (num_bytes < offs[T]) return stark_reject(GL_CHECK_TRUNCATED, check);
    if (num_bytes > offs[T]) return stark_reject(GL_CHECK_LENGTH, check);
    // get_challenges (get_challenges.rs:18-49): every trace cap in table order, then the CTL challenges
    gl_challenger ch{glhost::HostChallenger(p0.hasher)};
    std::vector<gl_t> cap(4 * ncap);
    for (uint32_t t = 0; t < T; t++) {
        VCursor cur{proof_bytes + offs[t], offs[t + 1] - offs[t]};
        cur.hashes(p0.hasher, cap.data(), ncap);
        ch.ch.observe_hashes(p0.hasher, cap.data(), ncap);
    }
    gl_t ctl_ch[2 * GL_STARK_MAX_CHALLENGES];
    for (uint32_t i = 0; i < 2 * nc; i++) ctl_ch[i] = ch.ch.challenge();
    // verify_stark_proof_with_challenges (verifier.rs:101-216) per table on the transcript running on: the vanishing identity, then its FRI
    std::vector<std::vector<gl_t>> lasts(T);
    StarkClaim claim;
    for (uint32_t t = 0; t < T; t++) {
        if (table) *table = t;
        TableCtl ctl;
        ctl.table = t; ctl.nctl = (uint32_t)sh.ctl_zs[t].size(); ctl.challenges = ctl_ch; ctl.desc = desc; ctl.shape = &sh;
        GL_TRY(verify_table(d.tables[t], sh.shapes[t], dags && dags[t] ? &sh.progs[t] : nullptr, d.params[t], &ctl, proof_bytes + offs[t], offs[t + 1] - offs[t],
                            offs[t + 1] - offs[t], ch, claim, check));
        lasts[t].swap(claim.ctl_zs_last);
    }
    // verify_cross_table_lookups (cross_table_lookup.rs:542-569)
    if (table) *table = T;
    size_t at[GL_STARK_SET_MAX_TABLES] = {0}, twc = 0;
    for (uint32_t l = 0; l < d.num_lookups; l++) {
        const uint32_t looking = d.lookup_num_looking[l];
        for (uint32_t chal = 0; chal < nc; chal++) {
            gl_t prod = 1;
            for (uint32_t k = 0; k < looking; k++) { const uint32_t tb = d.twc_table[twc + k]; prod = gl_mul(prod, lasts[tb][at[tb]++]); }
            const uint32_t tb = d.twc_table[twc + looking];
            if (gl_canon(prod) != gl_canon(lasts[tb][at[tb]++])) return stark_reject(GL_CHECK_CTL, check);
        }
        twc += looking + 1;
    }
    return GL_OK;
}

}  // namespace
