// What stark.hip shares with stark_set.hip: the checked description's shape, the gl_stark handle and the single-table phases a table
// set runs per table.  Host code.
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
    size_t n = 0, size = 0;
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
// eval_vanishing_poly at zeta over the extension field: the Stark's constraints, then the permutation checks (accs[num_challenges])
// (prog: the table's compiled DAG in place of the term list, or null)
void vanishing_at(const gl_stark_desc& d, const StarkShape& s, const gl2_t* local, const gl2_t* next, const gl_t* pub, const gl_t* alphas, gl2_t z_last,
                  gl2_t l_first, gl2_t l_last, const gl2_t* zs, const gl2_t* zs_next, const gl_t* sets, gl2_t* accs, const DagProgram* prog = nullptr);

// dag / prog: the table's constraints as a gl_stark_dag beside a desc without a term list, compiled into prog (both null: the term list)
int stark_check(const gl_stark_desc* desc, const gl_fri_params* params, StarkShape* shape, bool prover = true, const gl_stark_dag* dag = nullptr,
                DagProgram* prog = nullptr);
int stark_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, gl_stark** out);
// what stark_host_stage leaves of a proof for verify_fri_proof: the oracles' caps, the openings in FriOpenings order, the transcript where
// gl_verify_openings takes it over, zeta and g zeta, and the FriProof inside the proof bytes
struct StarkClaim {
    std::vector<gl_t> caps, openings;
    gl_challenger ch{glhost::HostChallenger(GL_HASHER_POSEIDON)};
    uint64_t points[2][2] = {};
    const uint8_t* fri = nullptr; size_t fri_len = 0;
};
int stark_host_stage(const gl_stark_desc& d, const StarkShape& s, const DagProgram* prog, const gl_fri_params& p, const uint8_t* proof_bytes, size_t num_bytes,
                     StarkClaim& out, uint32_t* check);
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
// ctl_zs: polynomials the Z batch holds after the permutation Zs (a set's CTL Zs)
int quotient_phase(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges, const uint64_t* alphas,
                   const uint64_t* public_inputs, DevBuf& d_q, uint32_t ctl_zs = 0);
int quotient_commit(gl_ctx* ctx, const gl_stark* s, DevBuf& d_q, gl_batch** quotient);
void seg_products_scan(hipStream_t st, const gl_t* d_fac, uint32_t n, uint32_t nz, gl_t* d_seg);

}  // namespace glstark
