// STARK constraints as an expression DAG (gl_stark_dag, include/plonky2_mi355x.h): the DAG's own rules, its
// compilation into the instruction stream both interpreters run -- the scheduler and a linear-scan slot allocator, host code -- the
// host interpreter over the extension field for the verifiers, and the launch of k_stark_quotient_dag.  Everything else a table in
// DAG form needs is stark.hip's and stark_set.hip's code, which dispatch here.
#include "stark_internal.hpp"
#include "stark_dag_kernels.cuh"
#include <algorithm>
#include <cstring>
#include <queue>

using namespace glstark;

namespace {

constexpr uint32_t DEGREE_SATURATED = 1u << 20;     // far above every bound, far below overflow when two are added

}  // namespace

int glstark::dag_compile(const gl_stark_desc* desc, const gl_stark_dag* dag, DagProgram* prog) {
    GL_REQUIRE(desc && dag, GL_ERR_ARG, "gl_stark_dag: null description / dag");
    const gl_stark_desc& d = *desc; const gl_stark_dag& g = *dag;
    GL_REQUIRE(d.num_columns >= 1 && d.num_columns <= GL_STARK_MAX_COLUMNS, GL_ERR_ARG, "gl_stark: 1..1024 columns");
    GL_REQUIRE(d.num_public_inputs <= GL_STARK_MAX_PUBLIC_INPUTS, GL_ERR_ARG, "gl_stark: at most 256 public inputs");
    GL_REQUIRE(d.constraint_degree >= 1 && d.constraint_degree <= GL_STARK_MAX_DEGREE, GL_ERR_ARG, "gl_stark: constraint degree is 1..9");
    GL_REQUIRE(g.num_nodes <= GL_STARK_DAG_MAX_NODES, GL_ERR_ARG, "gl_stark_dag: at most 65536 nodes");
    GL_REQUIRE(!g.num_nodes || (g.node_op && g.node_a && g.node_b), GL_ERR_ARG, "gl_stark_dag: null node table");
    GL_REQUIRE(g.num_constants <= GL_STARK_DAG_MAX_CONSTANTS, GL_ERR_ARG, "gl_stark_dag: at most 65536 constants");
    GL_REQUIRE(!g.num_constants || g.constants, GL_ERR_ARG, "gl_stark_dag: null constants table");
    GL_REQUIRE(g.num_constraints >= 1 && g.num_constraints <= GL_STARK_MAX_CONSTRAINTS, GL_ERR_ARG, "gl_stark_dag: 1..4096 constraints");
    GL_REQUIRE(g.constraint_filter && g.constraint_operand, GL_ERR_ARG, "gl_stark_dag: null constraint table");
    const uint32_t N = g.num_nodes, C = g.num_constraints, q = d.constraint_degree > 2 ? d.constraint_degree - 1 : 1;
    // the rules every operand word obeys; `defined` nodes exist where it stands -> its degree
    std::vector<uint32_t> degree(N);
    uint32_t operand_degree = 0;
    auto operand = [&](uint32_t w, uint32_t defined) -> int {
        const uint32_t kind = w >> 28, idx = w & 0x0FFFFFFFu;
        GL_REQUIRE(kind <= GL_STARK_CONST, GL_ERR_ARG, "gl_stark_dag: unknown operand kind");
        if (kind == GL_STARK_LOCAL || kind == GL_STARK_NEXT) { GL_REQUIRE(idx < d.num_columns, GL_ERR_ARG, "gl_stark_dag: column index out of range"); operand_degree = 1; }
        else if (kind == GL_STARK_PUBLIC) { GL_REQUIRE(idx < d.num_public_inputs, GL_ERR_ARG, "gl_stark_dag: public-input index out of range"); operand_degree = 0; }
        else if (kind == GL_STARK_CONST) { GL_REQUIRE(idx < g.num_constants, GL_ERR_ARG, "gl_stark_dag: constant index out of range"); operand_degree = 0; }
        else {
            GL_REQUIRE(idx < N, GL_ERR_ARG, "gl_stark_dag: node index out of range");
            GL_REQUIRE(idx < defined, GL_ERR_ARG, "gl_stark_dag: a NODE operand names no earlier node (forward or self reference)");
            operand_degree = degree[idx];
        }
        return GL_OK;
    };
    for (uint32_t k = 0; k < N; k++) {
        GL_REQUIRE(g.node_op[k] <= GL_STARK_OP_MUL, GL_ERR_ARG, "gl_stark_dag: unknown op");
        GL_TRY(operand(g.node_a[k], k));
        const uint32_t da = operand_degree;
        GL_TRY(operand(g.node_b[k], k));
        degree[k] = std::min(g.node_op[k] == GL_STARK_OP_MUL ? da + operand_degree : std::max(da, operand_degree), DEGREE_SATURATED);
    }
    DagProgram p;
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t filt = g.constraint_filter[c];
        GL_REQUIRE(filt <= GL_STARK_LAST_ROW, GL_ERR_ARG, "gl_stark_dag: unknown constraint filter");
        GL_TRY(operand(g.constraint_operand[c], N));
        // quotient degree < q n: as for a term of the term list (stark.hip), counted formally
        GL_REQUIRE(operand_degree <= ((filt == GL_STARK_FIRST_ROW || filt == GL_STARK_LAST_ROW) ? q : q + 1), GL_ERR_ARG,
                   "gl_stark_dag: a constraint's degree is above the constraint degree");
        p.max_degree = std::max(p.max_degree, operand_degree);
    }
    auto node_of = [](uint32_t w, uint32_t* idx) { *idx = w & 0x0FFFFFFFu; return (w >> 28) == GL_STARK_NODE; };
    // a node no constraint reaches is dropped
    std::vector<uint8_t> used(N, 0);
    uint32_t j = 0;
    for (uint32_t c = 0; c < C; c++) if (node_of(g.constraint_operand[c], &j)) used[j] = 1;
    for (uint32_t k = N; k-- > 0;) {
        if (!used[k]) continue;
        if (node_of(g.node_a[k], &j)) used[j] = 1;
        if (node_of(g.node_b[k], &j)) used[j] = 1;
    }
    // positions: 0 before node 0, 2 k + 1 node k, 2 k + 2 right after it.  Constraint c is consumed at the first position at which its
    // value exists and constraint c - 1 has been consumed.
    std::vector<uint32_t> emit_at(C), last_use(N, 0);
    {
        uint32_t c = 0;
        auto flush = [&](uint32_t defined, uint32_t pos) {
            for (; c < C; c++) {
                if (node_of(g.constraint_operand[c], &j)) { if (j >= defined) break; last_use[j] = std::max(last_use[j], pos); }
                emit_at[c] = pos;
            }
        };
        flush(0, 0);
        for (uint32_t k = 0; k < N; k++) {
            if (used[k]) {
                if (node_of(g.node_a[k], &j)) last_use[j] = std::max(last_use[j], 2 * k + 1);
                if (node_of(g.node_b[k], &j)) last_use[j] = std::max(last_use[j], 2 * k + 1);
            }
            flush(k + 1, 2 * k + 2);
        }
        GL_REQUIRE(c == C, GL_ERR_INTERNAL, "gl_stark_dag: the scheduler left a constraint behind");
    }
    // linear scan: an operand that dies at node k gives its slot back before node k takes one (the lowest free)
    std::vector<uint32_t> slot(N, 0);
    std::priority_queue<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> free_slots;
    uint32_t next_slot = 0, live = 0, c = 0;
    auto word = [&](uint32_t w) { return node_of(w, &j) ? GL_STARK_OPERAND(GL_STARK_NODE, slot[j]) : w; };
    auto release = [&](uint32_t w, uint32_t pos) { if (node_of(w, &j) && last_use[j] == pos) { last_use[j] = 0xFFFFFFFFu; free_slots.push(slot[j]); live--; } };
    auto emit = [&](uint32_t pos) {
        const uint32_t first = c;
        for (; c < C && emit_at[c] == pos; c++) { p.instr.insert(p.instr.end(), {GLS_DAG_EMIT | g.constraint_filter[c] << 8, word(g.constraint_operand[c]), 0u, 0u}); }
        for (uint32_t e = first; e < c; e++) release(g.constraint_operand[e], pos);
    };
    emit(0);
    for (uint32_t k = 0; k < N; k++) {
        if (used[k]) {
            const uint32_t a = word(g.node_a[k]), b = word(g.node_b[k]);
            release(g.node_a[k], 2 * k + 1);
            release(g.node_b[k], 2 * k + 1);                // x * x with x dying: released once (last_use is spent)
            if (free_slots.empty()) slot[k] = next_slot++; else { slot[k] = free_slots.top(); free_slots.pop(); }
            live++;
            p.max_live = std::max(p.max_live, live);
            p.instr.insert(p.instr.end(), {g.node_op[k] | slot[k] << 8, a, b, 0u});
        }
        emit(2 * k + 2);
    }
    GL_REQUIRE(next_slot == p.max_live && live == 0, GL_ERR_INTERNAL, "gl_stark_dag: the slot allocator and the liveness count disagree");
    GL_REQUIRE(p.max_live <= GL_STARK_DAG_MAX_LIVE, GL_ERR_ARG, "gl_stark_dag: more than 128 values live at once (GL_STARK_DAG_MAX_LIVE)");
    p.num_instructions = (uint32_t)(p.instr.size() / 4); p.num_constraints = C;
    p.constants.resize(g.num_constants);
    for (uint32_t i = 0; i < g.num_constants; i++) p.constants[i] = gl_canon(g.constants[i]);
    if (prog) *prog = std::move(p);
    return GL_OK;
}

// the host interpreter of the compiled program over the extension field: every constraint's value under its filter, in order
void glstark::dag_constraints_at(const DagProgram& prog, const gl2_t* local, const gl2_t* next, const gl_t* pub, gl2_t z_last, gl2_t l_first, gl2_t l_last,
                                 const std::function<void(gl2_t)>& consume) {
    std::vector<gl2_t> slots(prog.max_live + 1);
    auto value = [&](uint32_t w) {
        const uint32_t kind = w >> 28, idx = w & 0x0FFFFFFFu;
        return kind == GL_STARK_NODE ? slots[idx] : kind == GL_STARK_LOCAL ? local[idx] : kind == GL_STARK_NEXT ? next[idx] : kind == GL_STARK_CONST ? e_of(prog.constants[idx]) : e_of(pub[idx]);
    };
    for (uint32_t k = 0; k < prog.num_instructions; k++) {
        const uint32_t w0 = prog.instr[4 * k], op = w0 & 0xFFu, slot = w0 >> 8;
        const gl2_t a = value(prog.instr[4 * k + 1]);
        if (op == GLS_DAG_EMIT) {
            consume(slot == GL_STARK_TRANSITION ? gl2_mul(a, z_last) : slot == GL_STARK_FIRST_ROW ? gl2_mul(a, l_first) : slot == GL_STARK_LAST_ROW ? gl2_mul(a, l_last) : a);
            continue;
        }
        const gl2_t b = value(prog.instr[4 * k + 2]);
        slots[slot] = op == GL_STARK_OP_MUL ? gl2_mul(a, b) : op == GL_STARK_OP_ADD ? gl2_add(a, b) : gl2_sub(a, b);
    }
}

int glstark::quotient_dag_launch(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const gl_t* d_ch, const uint64_t* alphas,
                                 const gl_t* d_pub, gl_t* d_out) {
    GL_REQUIRE(s->dag && s->dag_max_live <= GL_STARK_DAG_MAX_LIVE, GL_ERR_INTERNAL, "gl_stark: no compiled DAG on this handle");
    GlStarkQuotDag q;
    ::memset((void*)&q, 0, sizeof q);
    q.trace = trace->lde; q.zs = zs ? zs->lde : nullptr; q.stride = trace->N();
    GL_REQUIRE((reinterpret_cast<uintptr_t>(s->d_dag_instr) & 15) == 0, GL_ERR_INTERNAL, "gl_stark: the compiled DAG is not 16-byte aligned");
    q.instr = reinterpret_cast<const uint4*>(s->d_dag_instr); q.constants = s->d_dag_const;
    q.pub = d_pub; q.ch = d_ch; q.pair_off = s->d_pair_off; q.pair_cols = s->d_pair_cols;
    q.xpow_lo = s->xt.lo; q.xpow_hi = s->xt.hi; q.lfirst = s->d_lagrange; q.llast = s->d_lagrange + s->size; q.out = d_out;
    for (uint32_t j = 0; j < s->nc; j++) q.alphas[j] = gl_canon(alphas[j]);
    for (int i = 0; i < 8; i++) q.zh_inv[i] = s->zh_inv[i];
    q.last = s->last;
    q.size = (uint32_t)s->size; q.step = 1u << (s->params.rate_bits - s->s.qdb); q.next_step = 1u << s->s.qdb;
    q.num_instructions = s->dag_num_instructions; q.nc = s->nc; q.q = s->s.q; q.nz = zs ? s->s.nz : 0; q.num_instances = s->s.num_instances;
    const dim3 grid((unsigned)((s->size + GLS_DAG_BLOCK - 1) / GLS_DAG_BLOCK)), block(GLS_DAG_BLOCK);
    const size_t lds = (size_t)s->dag_max_live * GLS_DAG_BLOCK * sizeof(gl_t);       // the program's own max live: a small one keeps its occupancy
    ctx->timing_begin("compute quotient polys");
    switch (s->nc) {
        case 1: hipLaunchKernelGGL(k_stark_quotient_dag<1>, grid, block, lds, ctx->stream, q); break;
        case 2: hipLaunchKernelGGL(k_stark_quotient_dag<2>, grid, block, lds, ctx->stream, q); break;
        case 3: hipLaunchKernelGGL(k_stark_quotient_dag<3>, grid, block, lds, ctx->stream, q); break;
        default: hipLaunchKernelGGL(k_stark_quotient_dag<4>, grid, block, lds, ctx->stream, q); break;
    }
    ctx->timing_end();
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}

extern "C" int gl_stark_dag_check(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params) try {
    GL_REQUIRE(dag, GL_ERR_ARG, "gl_stark_dag_check: null dag (gl_stark_check takes a term list)");
    return stark_check(desc, params, nullptr, true, dag, nullptr);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_dag_stats(const gl_stark_desc* desc, const gl_stark_dag* dag, uint32_t* max_live, uint32_t* max_degree, uint32_t* num_instructions) try {
    DagProgram prog;
    GL_TRY(dag_compile(desc, dag, &prog));
    if (max_live) *max_live = prog.max_live;
    if (max_degree) *max_degree = prog.max_degree;
    if (num_instructions) *num_instructions = prog.num_instructions;
    return GL_OK;
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_dag_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, gl_stark** out) try {
    GL_REQUIRE(out, GL_ERR_ARG, "gl_stark_dag_create: null out");
    *out = nullptr;
    GL_REQUIRE(dag, GL_ERR_ARG, "gl_stark_dag_create: null dag (gl_stark_create takes a term list)");
    return stark_create(ctx, desc, dag, params, out);
} catch (...) { return gl_caught(); }

extern "C" int gl_stark_dag_verify(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes,
                                   uint32_t* check) try {
    if (check) *check = GL_CHECK_ACCEPTED;
    GL_REQUIRE(dag, GL_ERR_ARG, "gl_stark_dag_verify: null dag (gl_stark_verify takes a term list)");
    return stark_verify(desc, dag, params, proof_bytes, num_bytes, check);
} catch (...) { return gl_caught(); }
