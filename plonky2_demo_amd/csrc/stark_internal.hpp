// What stark.hip shares with stark_set.hip: the checked description's shape, the gl_stark handle, the phases, and the one per-table
// prover body and verification stage that a single table and every table of a set go through.  Host code.
#pragma once
#include "context.hpp"
#include "fri_instance.hpp"
#include <functional>
#include <vector>

struct StarkShape {             // what stark.rs:79-221 derives from the description
    uint32_t q = 0, qdb = 0, num_instances = 0, nz = 0;
    size_t terms = 0, factors = 0, column_pairs = 0;
};

// A gl_stark_dag compiled (stark_dag.hip): the scheduler's instruction stream over the slot allocator's slots.  Four words an
// instruction (one aligned 16-byte scalar load on the device): op | dst_slot << 8 (op GL_STARK_OP_* ; GLS_DAG_EMIT carries the filter
// where the slot stands), then the operands a, b as kind << 28 | index with GL_STARK_NODE's index a SLOT and GL_STARK_CONST's an index
// into the canonical constants, then 0.
#define GLS_DAG_EMIT 3u
struct DagProgram {
    std::vector<uint32_t> instr;    // [num_instructions][4]
    std::vector<gl_t> constants;    // canonical
    uint32_t num_instructions = 0, num_constraints = 0, max_live = 0, max_degree = 0;
};

struct gl_stark {
    gl_ctx* ctx = nullptr;
    gl_fri_params params;
    StarkShape s;
    uint32_t num_columns = 0, num_public_inputs = 0, nc = 0, num_constraints = 0;
    size_t n = 0, size = 0, proof_bytes = 0;        // proof_bytes: the single-table proof's (table_proof_bytes without CTL Zs)
    void* d_tables = nullptr;   // one block: the term program, the pair tables, Z_H on the coset
    const uint32_t* d_filter = nullptr; const uint32_t* d_num_terms = nullptr; const uint32_t* d_term_nf = nullptr; const uint32_t* d_factors = nullptr;
    const uint32_t* d_pair_off = nullptr; const uint32_t* d_pair_cols = nullptr;
    const gl_t* d_coeff = nullptr;
    gl_t* d_lagrange = nullptr; // L_first | L_last on the quotient coset, [2][size]
    gl_t zh_inv[8] = {0}, last = 0, n_inv = 0;
    GlPowTable xt;              // 7 w_size^i
    // the DAG form (gl_stark_dag_create): the compiled program in d_tables in place of the term program
    bool dag = false;
    const uint32_t* d_dag_instr = nullptr; const gl_t* d_dag_const = nullptr;
    uint32_t dag_num_instructions = 0, dag_max_live = 0;
};

namespace glstark {

struct VCursor {                                       // little-endian reader over the proof bytes
    const uint8_t* p; size_t len, pos = 0;
    uint64_t u64() { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[pos + i] << (8 * i); pos += 8; return v; }
    void words(gl_t* out, size_t k) { for (size_t i = 0; i < k; i++) out[i] = gl_canon(u64()); }       // read_field takes a word mod p
    void hashes(uint32_t hasher, gl_t* out, size_t k) {
        if (hasher != GL_HASHER_KECCAK) { words(out, 4 * k); return; }
        for (size_t i = 0; i < k; i++) { for (int w = 0; w < 3; w++) out[4 * i + w] = u64(); out[4 * i + 3] = p[pos++]; }
    }
};
inline gl2_t e_of(gl_t v) { return gl2_make(gl_canon(v), 0); }
int stark_reject(uint32_t code, uint32_t* check);
gl2_t ext_pow2(gl2_t x, unsigned k);
struct TableCtl;
// eval_vanishing_poly at zeta over the extension field: the Stark's constraints, the permutation checks, then a set's CTL checks
// (accs[num_challenges]; prog: the table's compiled DAG in place of the term list, or null)
void vanishing_at(const gl_stark_desc& d, const StarkShape& s, const gl2_t* local, const gl2_t* next, const gl_t* pub, const gl_t* alphas, gl2_t z_last,
                  gl2_t l_first, gl2_t l_last, const gl2_t* zs, const gl2_t* zs_next, const gl_t* sets, gl2_t* accs, const DagProgram* prog = nullptr,
                  const TableCtl* ctl = nullptr);

// dag / prog: the table's constraints as a gl_stark_dag beside a desc without a term list, compiled into prog (both null: the term list)
int stark_check(const gl_stark_desc* desc, const gl_fri_params* params, StarkShape* shape, bool prover = true, const gl_stark_dag* dag = nullptr,
                DagProgram* prog = nullptr);
int stark_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, gl_stark** out);
// ---- one table's proof, alone (starky) or in a set (evm/src): the set's tables carry nctl CTL Zs behind their permutation Zs ----
// A table's place in a set (stark_set.hip fills it and defines what takes it, beside the CTL kernels); null stands for a single table.
struct SetShape;
struct TableCtl {
    uint32_t table = 0, nctl = 0;
    const uint64_t* challenges = nullptr;              // [num_challenges][2]: the set's beta, gamma
    const gl_stark_set* set = nullptr;                 // the prover's: the device CTL programs
    const gl_stark_set_desc* desc = nullptr; const SetShape* shape = nullptr;      // the verifier's: the checked description
};
inline uint32_t nctl_of(const TableCtl* ctl) { return ctl ? ctl->nctl : 0; }
// partial_products of the table's CTL Zs: d_trace VALUES [num_columns][n] -> d_z VALUES [nctl][n]
int ctl_z_values(gl_ctx* ctx, const TableCtl& ctl, const gl_t* d_trace, gl_t* d_z);
// the CTL checks folded into d_q behind k_stark_quotient's (zs: the whole Z batch)
int ctl_quotient_pass(gl_ctx* ctx, const TableCtl& ctl, const gl_batch* trace, const gl_batch* zs, const uint64_t* alphas, DevBuf& d_q);
// eval_cross_table_lookup_checks at zeta, consumed in order (zs, zs_next: the nctl CTL Zs' openings)
void ctl_checks_at(const TableCtl& ctl, const gl2_t* local, const gl2_t* next, const gl2_t* zs, const gl2_t* zs_next, gl2_t l_first, gl2_t z_last,
                   const std::function<void(gl2_t)>& consume);

// The table's FriInstanceInfo (starky/src/stark.rs:88-137, evm/src/stark.rs:83-142) at this proof's zeta: oracles trace, Z (permutation Zs,
// then CTL Zs; absent where there are none), quotient; batches [trace, Z, quotient] at zeta, [trace, Z] at g zeta and -- with CTL Zs --
// [CTL Zs] at g^-1.  The validation builds it at a zeta off the base field, which passes the points' coset check.
struct StarkInstance {
    gl_fri_instance inst;
    std::vector<uint32_t> polys;
    StarkInstance(const StarkInstance&) = delete;
    StarkInstance(uint32_t num_columns, uint32_t num_challenges, const StarkShape& s, uint32_t nctl, uint32_t degree_bits, gl2_t zeta = gl2_make(0, 1));
};
// the table's proof: caps, openings, ctl_zs_last, the FriProof (glfri::proof_bytes on the instance), public inputs
size_t table_proof_bytes(const gl_fri_params& p, uint32_t num_columns, uint32_t num_public_inputs, uint32_t nc, const StarkShape& s, uint32_t nctl);
// The prover from where the trace cap stands in the proof and in the transcript (a set's compact() done) to the public inputs, appended to o:
// prover.rs:76-194, evm/src/prover.rs:288-467.  who: the entry's name in the messages.
int prove_table(gl_ctx* ctx, const gl_stark* s, const TableCtl* ctl, const uint64_t* d_cols, const gl_batch* trace, const uint64_t* h_public_inputs, gl_challenger& ch,
                std::vector<uint8_t>& o, const char* who);
// what stark_host_stage leaves of a table's proof for verify_fri_proof: the oracles' caps, the openings in FriOpenings order, zeta, g zeta and
// g^-1, the FriProof inside the proof bytes; and ctl_zs_last for the product across the tables
struct StarkClaim {
    std::vector<gl_t> caps, openings, ctl_zs_last;
    uint64_t points[3][2] = {};
    const uint8_t* fri = nullptr; size_t fri_len = 0;
};
// A table's proof up to its final gl_verify_openings, for a description that passed stark_check (prog: its compiled DAG, or null): the
// byte count against total (the table's table_proof_bytes, which every caller has), caps, openings, get_challenges on ch -- a single table's
// starts there, a set's runs on from table to table --, the vanishing identity
int stark_host_stage(const gl_stark_desc& d, const StarkShape& s, const DagProgram* prog, const gl_fri_params& p, const TableCtl* ctl, const uint8_t* proof_bytes,
                     size_t num_bytes, size_t total, gl_challenger& ch, StarkClaim& out, uint32_t* check);
// the stage, then verify_fri_proof on the table's instance at this proof's points
int verify_table(const gl_stark_desc& d, const StarkShape& s, const DagProgram* prog, const gl_fri_params& p, const TableCtl* ctl, const uint8_t* proof_bytes,
                 size_t num_bytes, size_t total, gl_challenger& ch, StarkClaim& claim, uint32_t* check);
int stark_verify(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check);
// stark_dag.hip: the DAG's own rules and its compilation; the constraints of a compiled program at zeta, consumed in order; the launch
// of k_stark_quotient_dag with everything k_stark_quotient takes
int dag_compile(const gl_stark_desc* desc, const gl_stark_dag* dag, DagProgram* prog);
void dag_constraints_at(const DagProgram& prog, const gl2_t* local, const gl2_t* next, const gl_t* pub, gl2_t z_last, gl2_t l_first, gl2_t l_last,
                        const std::function<void(gl2_t)>& consume);
int quotient_dag_launch(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const gl_t* d_ch, const uint64_t* alphas, const gl_t* d_pub,
                        gl_t* d_out);
int check_stark_batch(const gl_stark* s, const gl_batch* b, size_t ncols, const char* what);
int upload_challenges(gl_ctx* ctx, const gl_stark* s, const uint64_t* challenges, DevBuf& d_ch);
int read_flag(gl_ctx* ctx, const uint32_t* d_flag, uint32_t* flag);
int permutation_z_values(gl_ctx* ctx, const gl_stark* s, const gl_t* d_trace, const gl_t* d_ch, gl_t* d_z);
// the Z phase: permutation Zs, then the table's CTL Zs, committed as one batch
int zs_commit(gl_ctx* ctx, const gl_stark* s, const TableCtl* ctl, const uint64_t* d_trace_values, const uint64_t* challenges, gl_batch** zs);
// zs: the whole Z batch, null where the table has neither permutation pairs nor CTL Zs
int quotient_phase(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges, const uint64_t* alphas,
                   const uint64_t* public_inputs, DevBuf& d_q, const TableCtl* ctl = nullptr);
int quotient_commit(gl_ctx* ctx, const gl_stark* s, DevBuf& d_q, gl_batch** quotient);
void seg_products_scan(hipStream_t st, const gl_t* d_fac, uint32_t n, uint32_t nz, gl_t* d_seg);

}  // namespace glstark
