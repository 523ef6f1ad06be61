// STARK table sets (evm/src/cross_table_lookup.rs, evm/src/stark.rs:83-142): tables as gl_stark_desc tied by cross-table lookups handed
// over as data -- gl_stark_set_desc -- its validation, the CTL running products Z and the CTL checks of the quotient.  Per table
// everything else is stark.hip's single-table code.
#include "stark_internal.hpp"
#include "proof.hpp"
#include "stark_ctl_kernels.cuh"
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

using namespace glstark;

namespace {

struct CtlZ { uint32_t twc, chal; };            // one CTL Z of a table: its TableWithColumns and its challenge
struct SetShape {
    uint32_t num_tables = 0, nc = 0;
    std::vector<StarkShape> shapes;             // per table
    std::vector<std::vector<CtlZ>> ctl_zs;      // per table, in cross_table_lookup_data's order
    std::vector<uint32_t> col_off;              // [Columns + 1] start of each Column's terms
    std::vector<uint32_t> twc_col0;             // [twcs] first Column of each TableWithColumns
    std::vector<DagProgram> progs;              // per table: its compiled DAG where dags[t] is given (gl_stark_set_dag_*)
};

// the FriInstanceInfo of evm/src/stark.rs:83-142: oracles trace, Z (permutation Zs, then CTL Zs), quotient; batches [trace, Z, quotient] at
// zeta, [trace, Z] at g zeta and -- with CTL Zs -- [CTL Zs] at g^-1
struct StarkSetInstance {
    gl_fri_instance inst;
    std::vector<uint32_t> polys;
    StarkSetInstance(const StarkSetInstance&) = delete;
    StarkSetInstance(uint32_t num_columns, uint32_t num_challenges, const StarkShape& s, uint32_t nctl, gl2_t zeta, gl2_t zeta_next, gl_t g_inv) {
        ::memset((void*)&inst, 0, sizeof inst);
        const uint32_t nzs = s.nz + nctl, nq = s.q * num_challenges;
        inst.num_oracles = 3;
        inst.oracle_num_polys[0] = num_columns; inst.oracle_num_polys[1] = nzs; inst.oracle_num_polys[2] = nq;
        inst.num_batches = nctl ? 3 : 2;
        inst.points[0][0] = zeta.a; inst.points[0][1] = zeta.b; inst.points[1][0] = zeta_next.a; inst.points[1][1] = zeta_next.b;
        inst.points[2][0] = g_inv; inst.points[2][1] = 0;
        for (int b = 0; b < 2; b++) {
            const size_t before = polys.size() / 2;
            for (uint32_t c = 0; c < num_columns; c++) { polys.push_back(0); polys.push_back(c); }
            for (uint32_t c = 0; c < nzs; c++) { polys.push_back(1); polys.push_back(c); }
            if (b == 0) for (uint32_t c = 0; c < nq; c++) { polys.push_back(2); polys.push_back(c); }
            inst.batch_len[b] = (uint32_t)(polys.size() / 2 - before);
        }
        for (uint32_t c = 0; c < nctl; c++) { polys.push_back(1); polys.push_back(s.nz + c); }
        inst.batch_len[2] = nctl;
        inst.polys = polys.data();
    }
};

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
        const StarkSetInstance si(d.tables[t].num_columns, s.nc, s.shapes[t], (uint32_t)s.ctl_zs[t].size(), gl2_make(0, 1), gl2_make(0, 1),
                                  gl_canon(gl_inv(gl_host_root_of_unity(d.params[t].degree_bits))));
        GL_TRY(glfri::check(&d.params[t], &si.inst, prover));
    }
    if (shape) *shape = std::move(s);
    return GL_OK;
}

}  // namespace

struct gl_stark_set {
    gl_ctx* ctx = nullptr;
    uint32_t num_tables = 0, nc = 0;
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

// partial_products (cross_table_lookup.rs:279-306) of every CTL Z of a table: d_trace VALUES [num_columns][n] -> d_z VALUES [nctl][n]
int ctl_z_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_t* d_trace, const uint64_t* ctl_challenges, gl_t* d_z) {
    const gl_stark* st = s->tables[table];
    const uint32_t n = (uint32_t)st->n, nzc = s->nctl[table], nseg = (n + GLS_SEG - 1) / GLS_SEG;
    hipStream_t stream = ctx->stream;
    std::vector<gl_t> ch(2 * (size_t)s->nc);
    for (size_t i = 0; i < ch.size(); i++) ch[i] = gl_canon(ctl_challenges[i]);
    DevBuf d_ch(ctx), d_fac(ctx), d_seg(ctx), d_flag(ctx);
    GL_TRY(d_ch.alloc(ch.size() * sizeof(gl_t)));
    GL_TRY(gl_copy_h2d(ctx, d_ch.p, ch.data(), ch.size() * sizeof(gl_t)));
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

}  // namespace

extern "C" int gl_stark_set_ctl_z_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* ctl_challenges,
                                         uint64_t* h_out) try {
    GL_TRY(check_set_args(ctx, s, table));
    GL_REQUIRE(d_trace_values && ctl_challenges && h_out, GL_ERR_ARG, "gl_stark_set_ctl_z_values: null argument");
    GL_REQUIRE(s->nctl[table], GL_ERR_ARG, "gl_stark_set_ctl_z_values: the table stands in no cross-table lookup");
    const size_t bytes = (size_t)s->nctl[table] * s->tables[table]->n * sizeof(gl_t);
    DevBuf d_z(ctx);
    GL_TRY(d_z.alloc(bytes));
    GL_TRY(ctl_z_values(ctx, s, table, d_trace_values, ctl_challenges, d_z.as<gl_t>()));
    return gl_copy_d2h(ctx, h_out, d_z.p, bytes);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_set_zs(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* permutation_challenges,
                               const uint64_t* ctl_challenges, gl_batch** zs) try {
    GL_REQUIRE(zs, GL_ERR_ARG, "gl_stark_set_zs: null out");
    *zs = nullptr;
    GL_TRY(check_set_args(ctx, s, table));
    const gl_stark* st = s->tables[table];
    const uint32_t nz = st->s.nz, nzc = s->nctl[table];
    GL_REQUIRE(d_trace_values && (ctl_challenges || !nzc), GL_ERR_ARG, "gl_stark_set_zs: null argument");
    GL_REQUIRE((nz != 0) == (permutation_challenges != nullptr), GL_ERR_ARG, "gl_stark_set_zs: the permutation challenge sets go with permutation pairs (null without)");
    DevBuf d_ch(ctx), d_z(ctx);
    GL_TRY(d_z.alloc((size_t)(nz + nzc) * st->n * sizeof(gl_t)));
    if (nz) {
        GL_TRY(upload_challenges(ctx, st, permutation_challenges, d_ch));
        GL_TRY(permutation_z_values(ctx, st, d_trace_values, d_ch.as<const gl_t>(), d_z.as<gl_t>()));
    }
    if (nzc) GL_TRY(ctl_z_values(ctx, s, table, d_trace_values, ctl_challenges, d_z.as<gl_t>() + (size_t)nz * st->n));
    return gl_batch_from_device_h(ctx, st->params.hasher, d_z.as<uint64_t>(), nz + nzc, st->n, st->params.rate_bits, st->params.cap_height, 1, zs);
} catch (...) { return gl_caught(); }

namespace {

// the set's quotient values: k_stark_quotient on the table's own constraints and permutation checks, then the CTL checks folded in
int set_quotient_phase(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs, const uint64_t* permutation_challenges,
                       const uint64_t* ctl_challenges, const uint64_t* alphas, const uint64_t* public_inputs, DevBuf& d_q) {
    GL_TRY(check_set_args(ctx, s, table));
    const gl_stark* st = s->tables[table];
    const uint32_t nz = st->s.nz, nctl = s->nctl[table];
    GL_REQUIRE(zs && (ctl_challenges || !nctl), GL_ERR_ARG, "gl_stark_set quotient: null Z batch / CTL challenges");
    GL_REQUIRE((nz != 0) == (permutation_challenges != nullptr), GL_ERR_ARG, "gl_stark_set quotient: the permutation challenge sets go with permutation pairs (null without)");
    GL_TRY(check_stark_batch(st, zs, nz + nctl, "gl_stark_set quotient: the Z batch does not match the description / params (permutation Zs, then CTL Zs)"));
    GL_TRY(quotient_phase(ctx, st, trace, nz ? zs : nullptr, permutation_challenges, alphas, public_inputs, d_q, nctl));
    if (!nctl) return GL_OK;
    std::vector<gl_t> ch(2 * (size_t)s->nc);
    for (size_t i = 0; i < ch.size(); i++) ch[i] = gl_canon(ctl_challenges[i]);
    DevBuf d_ch(ctx);
    GL_TRY(d_ch.alloc(ch.size() * sizeof(gl_t)));
    GL_TRY(gl_copy_h2d(ctx, d_ch.p, ch.data(), ch.size() * sizeof(gl_t)));
    GlStarkQuotCtl q;
    ::memset((void*)&q, 0, sizeof q);
    q.c = s->prog[table];
    q.c.trace = trace->lde; q.c.ch = d_ch.as<const gl_t>(); q.c.n = 0;
    q.stride = trace->N(); q.zs = zs->lde + (size_t)nz * q.stride;
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

// the size of gl_prove_openings' FriProof on a table's instance: oracles of ncols, nzs and nq polynomials
size_t set_fri_proof_bytes(const gl_fri_params& p, uint32_t ncols, uint32_t nzs, uint32_t nq) {
    const size_t hb = hash_wire_bytes(p.hasher), lgN = p.degree_bits + p.rate_bits;
    size_t per_query = 0, lg = lgN, total_arity = 0;
    const uint32_t leaf[3] = {ncols, nzs, nq};
    for (int o = 0; o < 3; o++) per_query += 8 * (size_t)leaf[o] + 1 + hb * (lgN - p.cap_height);
    for (unsigned r = 0; r < p.num_fri_rounds; r++) {
        lg -= p.fri_arity_bits[r]; total_arity += p.fri_arity_bits[r];
        per_query += (size_t(16) << p.fri_arity_bits[r]) + 1 + hb * (lg - p.cap_height);
    }
    return (size_t)p.num_fri_rounds * (hb << p.cap_height) + (size_t)p.num_query_rounds * per_query + 16 * ((size_t(1) << p.degree_bits) >> total_arity) + 8;
}
size_t table_proof_bytes(const gl_fri_params& p, uint32_t ncols, uint32_t npi, uint32_t nc, const StarkShape& s, uint32_t nctl) {
    const uint32_t nzs = s.nz + nctl, nq = s.q * nc;
    return 3 * (hash_wire_bytes(p.hasher) << p.cap_height) + 16 * (2 * (size_t)ncols + 2 * (size_t)nzs + nq) + 8 * (size_t)nctl +
           set_fri_proof_bytes(p, ncols, nzs, nq) + 8 * (size_t)npi;
}
size_t set_proof_bytes(const gl_stark_set* s) {
    size_t total = 0;
    for (uint32_t t = 0; t < s->num_tables; t++) {
        const gl_stark* st = s->tables[t];
        total += table_proof_bytes(st->params, st->num_columns, st->num_public_inputs, st->nc, st->s, s->nctl[t]);
    }
    return total;
}

// prove_single_table (evm/src/prover.rs:288-467) from the compact on, appended to o
int prove_table(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_cols, const gl_batch* trace, const gl_t* trace_cap, const gl_t* ctl_ch,
                const uint64_t* h_public_inputs, gl_challenger& ch, std::vector<uint8_t>& o) {
    const gl_stark* st = s->tables[table];
    const gl_fri_params& p = st->params;
    const size_t ncap = size_t(1) << p.cap_height, start = o.size();
    const uint32_t nz = st->s.nz, nctl = s->nctl[table], nzs = nz + nctl, nq = st->s.q * st->nc, ncols = st->num_columns;
    GL_REQUIRE(h_public_inputs || !st->num_public_inputs, GL_ERR_ARG, "gl_stark_set_prove: null public inputs of a table that has some");
    std::vector<gl_t> cap(4 * ncap);
    BatchHolder zs, quot;
    put_hashes(o, p.hasher, trace_cap, ncap);
    ch.ch.compact();
    std::vector<gl_t> sets;
    if (nz) for (uint32_t i = 0; i < 2 * st->s.q * st->nc; i++) sets.push_back(ch.ch.challenge());
    GL_TRY(gl_stark_set_zs(ctx, s, table, d_cols, nz ? sets.data() : nullptr, ctl_ch, &zs.b));
    GL_TRY(gl_batch_cap(zs.b, cap.data()));
    put_hashes(o, p.hasher, cap.data(), ncap);
    ch.ch.observe_hashes(p.hasher, cap.data(), ncap);
    gl_t alphas[GL_STARK_MAX_CHALLENGES];
    for (uint32_t j = 0; j < st->nc; j++) alphas[j] = ch.ch.challenge();
    GL_TRY(gl_stark_set_quotient_polys(ctx, s, table, trace, zs.b, nz ? sets.data() : nullptr, ctl_ch, alphas, h_public_inputs, &quot.b));
    GL_TRY(gl_batch_cap(quot.b, cap.data()));
    put_hashes(o, p.hasher, cap.data(), ncap);
    ch.ch.observe_hashes(p.hasher, cap.data(), ncap);
    const gl2_t zeta = ch.ch.challenge_ext();
    const gl2_t zn = ext_pow2(zeta, p.degree_bits);
    GL_REQUIRE(!(zn.a == 1 && zn.b == 0), GL_ERR_ZETA_IN_SUBGROUP, "gl_stark_set_prove: opening point is in the subgroup");
    const gl_t g = gl_host_root_of_unity(p.degree_bits), g_inv = gl_canon(gl_inv(g));
    const gl2_t zeta_next = gl2_canon(gl2_scalar(zeta, g));
    const gl_t zw[2] = {zeta.a, zeta.b}, znw[2] = {zeta_next.a, zeta_next.b}, lw[2] = {g_inv, 0};
    // StarkOpeningSet::new (evm/src/proof.rs:224-259)
    std::vector<gl_t> local(2 * ncols), next(2 * ncols), zl(2 * nzs), zn_(2 * nzs), last(2 * nctl + 2), ql(2 * nq);
    GL_TRY(gl_open_at(ctx, trace, zw, 0, ncols, local.data()));
    GL_TRY(gl_open_at(ctx, trace, znw, 0, ncols, next.data()));
    GL_TRY(gl_open_at(ctx, zs.b, zw, 0, nzs, zl.data()));
    GL_TRY(gl_open_at(ctx, zs.b, znw, 0, nzs, zn_.data()));
    if (nctl) GL_TRY(gl_open_at(ctx, zs.b, lw, nz, nctl, last.data()));
    GL_TRY(gl_open_at(ctx, quot.b, zw, 0, nq, ql.data()));
    for (uint32_t k = 0; k < nctl; k++) GL_REQUIRE(gl_canon(last[2 * k + 1]) == 0, GL_ERR_INTERNAL, "gl_stark_set_prove: a base-field opening left the base field");
    put_words(o, local.data(), local.size()); put_words(o, next.data(), next.size());
    put_words(o, zl.data(), zl.size()); put_words(o, zn_.data(), zn_.size());
    for (uint32_t k = 0; k < nctl; k++) put_u64(o, gl_canon(last[2 * k]));
    put_words(o, ql.data(), ql.size());
    // observe_openings(to_fri_openings): [local, zs, quotient], [next, zs_next], [ctl_zs_last lifted]
    ch.ch.observe_many(local.data(), local.size()); ch.ch.observe_many(zl.data(), zl.size()); ch.ch.observe_many(ql.data(), ql.size());
    ch.ch.observe_many(next.data(), next.size()); ch.ch.observe_many(zn_.data(), zn_.size());
    ch.ch.observe_many(last.data(), 2 * (size_t)nctl);
    const StarkSetInstance si(ncols, st->nc, st->s, nctl, zeta, zeta_next, g_inv);
    const gl_batch* batches[3] = {trace, zs.b, quot.b};
    const size_t at = o.size(), fri_len = set_fri_proof_bytes(p, ncols, nzs, nq);
    size_t fri_bytes = 0;
    o.resize(at + fri_len);
    GL_TRY(gl_prove_openings(ctx, &p, &si.inst, batches, &ch, o.data() + at, fri_len, &fri_bytes));
    GL_REQUIRE(fri_bytes == fri_len, GL_ERR_INTERNAL, "gl_stark_set_prove: the FriProof has another size than the params and the instance fix");
    for (uint32_t i = 0; i < st->num_public_inputs; i++) put_u64(o, gl_canon(h_public_inputs[i]));
    GL_REQUIRE(o.size() - start == table_proof_bytes(p, ncols, st->num_public_inputs, st->nc, st->s, nctl), GL_ERR_INTERNAL,
               "gl_stark_set_prove: a table's proof has another size than gl_stark_set_proof_size counts");
    return GL_OK;
}

int set_prove_device(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* d_cols, const uint64_t* const* h_public_inputs, uint8_t* h_out, size_t cap_bytes,
                     size_t* num_bytes) {
    GL_TRY(check_set_args(ctx, s, 0));
    GL_REQUIRE(d_cols && num_bytes, GL_ERR_ARG, "gl_stark_set_prove: null argument");
    const size_t total = set_proof_bytes(s);
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
    for (uint32_t t = 0; t < s->num_tables; t++)
        GL_TRY(prove_table(ctx, s, t, d_cols[t], traces[t].b, caps.data() + 4 * ncap * t, ctl_ch, h_public_inputs ? h_public_inputs[t] : nullptr, ch, o));
    GL_REQUIRE(o.size() == total, GL_ERR_INTERNAL, "gl_stark_set_prove: the proof has another size than gl_stark_set_proof_size");
    ::memcpy(h_out, o.data(), total);
    return GL_OK;
}

}  // namespace

extern "C" size_t gl_stark_set_proof_size(const gl_stark_set* s) noexcept { return s ? set_proof_bytes(s) : 0; }

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

namespace {

int set_verify(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check, uint32_t* table) {
    SetShape sh;
    GL_TRY(stark_set_check(desc, &sh, false, dags));
    GL_REQUIRE(proof_bytes || !num_bytes, GL_ERR_ARG, "gl_stark_set_verify: null proof");
    const gl_stark_set_desc& d = *desc;
    const uint32_t T = d.num_tables, nc = sh.nc;
    if (table) *table = T;
    const gl_fri_params& p0 = d.params[0];
    const size_t ncap = size_t(1) << p0.cap_height, hb = hash_wire_bytes(p0.hasher);
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
    std::vector<std::vector<gl_t>> lasts(T);
    for (uint32_t t = 0; t < T; t++) {
        if (table) *table = t;
        const gl_stark_desc& td = d.tables[t]; const gl_fri_params& p = d.params[t]; const StarkShape& s = sh.shapes[t];
        const uint32_t ncols = td.num_columns, nz = s.nz, nctl = (uint32_t)sh.ctl_zs[t].size(), nzs = nz + nctl, nq = s.q * nc;
        VCursor cur{proof_bytes + offs[t], offs[t + 1] - offs[t]};
        std::vector<gl_t> caps(4 * ncap * 3), pub(td.num_public_inputs + 1);
        cur.hashes(p.hasher, caps.data(), ncap * 3);
        const size_t nopen = 2 * (size_t)ncols + 2 * nzs + nq;
        std::vector<gl_t> w(2 * nopen - 2 * nq), wq(2 * (size_t)nq);
        cur.words(w.data(), w.size());
        lasts[t].resize(nctl);
        cur.words(lasts[t].data(), nctl);
        cur.words(wq.data(), wq.size());
        const gl2_t* ext = (const gl2_t*)w.data();
        const gl2_t *local = ext, *next = ext + ncols, *zl = ext + 2 * ncols, *zn = zl + nzs, *ql = (const gl2_t*)wq.data();
        const uint8_t* fri = proof_bytes + offs[t] + cur.pos;
        const size_t fri_len = set_fri_proof_bytes(p, ncols, nzs, nq);
        cur.pos += fri_len;
        cur.words(pub.data(), td.num_public_inputs);
        (void)hb;
        // StarkProof::get_challenges (get_challenges.rs:95-149) after the compact of :39
        ch.ch.compact();
        std::vector<gl_t> sets;
        if (nz) for (uint32_t i = 0; i < 2 * s.q * nc; i++) sets.push_back(ch.ch.challenge());
        ch.ch.observe_hashes(p.hasher, caps.data() + 4 * ncap, ncap);
        gl_t alphas[GL_STARK_MAX_CHALLENGES];
        for (uint32_t j = 0; j < nc; j++) alphas[j] = ch.ch.challenge();
        ch.ch.observe_hashes(p.hasher, caps.data() + 8 * ncap, ncap);
        const gl2_t zeta = ch.ch.challenge_ext();
        std::vector<gl_t> openings;
        openings.reserve(2 * nopen + 2 * nctl);
        auto push = [&](const gl2_t* v, size_t k) { for (size_t i = 0; i < k; i++) { openings.push_back(v[i].a); openings.push_back(v[i].b); } };
        push(local, ncols); push(zl, nzs); push(ql, nq); push(next, ncols); push(zn, nzs);
        for (uint32_t k = 0; k < nctl; k++) { openings.push_back(lasts[t][k]); openings.push_back(0); }
        ch.ch.observe_many(openings.data(), openings.size());
        // verify_stark_proof_with_challenges (verifier.rs:101-216): vanishing(zeta) = Z_H(zeta) t(zeta) per challenge
        const gl_t g = gl_host_root_of_unity(p.degree_bits), n_field = gl_t(1) << p.degree_bits, g_inv = gl_canon(gl_inv(g));
        const gl2_t one = gl2_make(1, 0);
        const gl2_t zeta_pow = ext_pow2(zeta, p.degree_bits), z_h = gl2_sub(zeta_pow, one);
        const gl2_t l_first = gl2_mul(z_h, gl2_inv(gl2_scalar(gl2_sub(zeta, one), n_field)));
        const gl2_t l_last = gl2_mul(z_h, gl2_inv(gl2_scalar(gl2_sub(gl2_scalar(zeta, g), one), n_field)));
        const gl2_t z_last = gl2_sub(zeta, e_of(g_inv));
        gl2_t accs[GL_STARK_MAX_CHALLENGES];
        vanishing_at(td, s, local, next, pub.data(), alphas, z_last, l_first, l_last, zl, zn, sets.data(), accs, dags && dags[t] ? &sh.progs[t] : nullptr);
        auto consume = [&](gl2_t c) { for (uint32_t j = 0; j < nc; j++) accs[j] = gl2_add(gl2_scalar(accs[j], alphas[j]), c); };
        // eval_cross_table_lookup_checks on the Zs after the permutation ones (CtlCheckVars::from_proofs, cross_table_lookup.rs:325-414)
        for (uint32_t k = 0; k < nctl; k++) {
            const CtlZ& z = sh.ctl_zs[t][k];
            const uint32_t c0 = sh.twc_col0[z.twc], nco = d.twc_num_columns[z.twc], has_filter = d.twc_has_filter[z.twc];
            const gl_t beta = gl_canon(ctl_ch[2 * z.chal]), gamma = gl_canon(ctl_ch[2 * z.chal + 1]);
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
                return gl2_sub(gl2_add(gl2_mul(f, comb), one), f);           // select(f, x) = f x + 1 - f
            };
            consume(gl2_mul(gl2_sub(zl[nz + k], selected(local)), l_first));
            consume(gl2_mul(gl2_sub(zn[nz + k], gl2_mul(zl[nz + k], selected(next))), z_last));
        }
        for (uint32_t j = 0; j < nc; j++) {
            gl2_t tq = gl2_make(0, 0);
            for (uint32_t k = s.q; k-- > 0;) tq = gl2_add(gl2_mul(tq, zeta_pow), ql[j * s.q + k]);
            const gl2_t lhs = gl2_canon(accs[j]), rhs = gl2_canon(gl2_mul(z_h, tq));
            if (lhs.a != rhs.a || lhs.b != rhs.b) return stark_reject(GL_CHECK_VANISHING, check);
        }
        const StarkSetInstance si(ncols, nc, s, nctl, zeta, gl2_canon(gl2_scalar(zeta, g)), g_inv);
        const int st = gl_verify_openings(&p, &si.inst, caps.data(), openings.data(), &ch, fri, fri_len, check);
        if (st != GL_OK) return st;
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
