// The quotient kernel of a STARK table whose constraints are an expression DAG (gl_stark_dag, include/plonky2_mi355x.h): the device
// interpreter of the program stark_dag.hip compiles.
//   k_stark_quotient_dag    sum_i alpha^i C_i(x) / Z_H(x) on the quotient coset: k_stark_quotient (stark_kernels.cuh) with the term loop
//                           replaced by the instruction loop; indexing, x, z_last, the L_first / L_last tables, the named accumulators,
//                           the permutation checks and the final 1 / Z_H are the same
// The instructions are read through kernel arguments and a loop counter only: every address is wave-uniform, the loads are scalar and
// every branch on an instruction is uniform.  Node values live in LDS, slot s of thread t at lds[s * GLS_DAG_BLOCK + t]: a wave's
// ds_read_b64 / ds_write_b64 touch 64 consecutive words (no bank conflict), a thread touches its own cells only (no barrier), and no
// value sits in a runtime-indexed private array (scratch on gfx950).  The launch sizes the LDS to the program's own max live.
#pragma once
#include "gl64.cuh"
#include "../../include/plonky2_mi355x.h"

#define GLS_DAG_BLOCK 64        // threads per workgroup: one wave, 512 B of LDS per slot
#define GLS_DAG_EMIT 3u         // the fourth opcode: consume operand a under the filter the slot field carries

struct GlStarkQuotDag {
    const gl_t* trace;          // trace LDE [num_columns][stride], natural order
    const gl_t* zs;             // Z LDE [nz][stride], or null without pairs
    uint64_t stride;            // n << rate_bits
    const uint4* instr;         // [num_instructions]: (op | slot << 8, a, b, 0), 16-byte aligned: one scalar load an instruction
                                // (operands kind << 28 | index; NODE's index is a slot)
    const gl_t* constants;      // canonical
    const gl_t* pub;            // [num_public_inputs] canonical
    const gl_t* ch;             // [q][num_challenges][2], canonical
    const uint32_t* pair_off; const uint32_t* pair_cols;
    const gl_t* xpow_lo; const gl_t* xpow_hi;   // 7 w_size^i two-level
    const gl_t* lfirst; const gl_t* llast;      // [size]
    gl_t* out;                  // [num_challenges][size]
    gl_t alphas[4];
    gl_t zh_inv[8];             // 1 / Z_H(x_i) by i mod 2^qdb
    gl_t last;                  // g^-1
    uint32_t size, step, next_step, num_instructions, nc, q, nz, num_instances;
};

// One thread per point i of the quotient coset, as k_stark_quotient.  Dynamic LDS: max_live * GLS_DAG_BLOCK words.
template <int NC>
__global__ __launch_bounds__(GLS_DAG_BLOCK) void k_stark_quotient_dag(GlStarkQuotDag p) {
    extern __shared__ gl_t gls_dag_slots[];
    const uint32_t i = blockIdx.x * GLS_DAG_BLOCK + threadIdx.x;
    if (i >= p.size) return;
    const size_t il = (size_t)i * p.step, in = (size_t)((i + p.next_step) & (p.size - 1)) * p.step;
    const gl_t x = gl_mul(p.xpow_lo[i & 2047], p.xpow_hi[i >> 11]);
    const gl_t z_last = gl_sub(x, p.last), lf = p.lfirst[i], ll = p.llast[i];
    gl_t* const mine = gls_dag_slots + threadIdx.x;
    gl_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#define GLS_CONSUME(C)                                                  \
    do {                                                                \
        const gl_t _c = (C);                                            \
        a0 = gl_mul_add(_c, a0, p.alphas[0]);                           \
        if (NC > 1) a1 = gl_mul_add(_c, a1, p.alphas[1]);               \
        if (NC > 2) a2 = gl_mul_add(_c, a2, p.alphas[2]);               \
        if (NC > 3) a3 = gl_mul_add(_c, a3, p.alphas[3]);               \
    } while (0)
#define GLS_OPERAND(V, W)                                                               \
    do {                                                                                \
        const uint32_t _w = (W), _kind = _w >> 28, _idx = _w & 0x0FFFFFFFu;             \
        if (_kind == GL_STARK_NODE) V = mine[_idx * GLS_DAG_BLOCK];                     \
        else if (_kind == GL_STARK_LOCAL) V = p.trace[(size_t)_idx * p.stride + il];    \
        else if (_kind == GL_STARK_NEXT) V = p.trace[(size_t)_idx * p.stride + in];     \
        else if (_kind == GL_STARK_CONST) V = p.constants[_idx];                        \
        else V = p.pub[_idx];                                                           \
    } while (0)
    // the Stark's own constraints: the compiled program, `op dst_slot, a, b` and `emit filter, a` (constraint_consumer.rs:53-76)
    for (uint32_t k = 0; k < p.num_instructions; k++) {
        const uint4 w = p.instr[k];
        const uint32_t op = w.x & 0xFFu, slot = w.x >> 8;
        gl_t a, b;
        GLS_OPERAND(a, w.y);
        if (op == GLS_DAG_EMIT) {
            if (slot == GL_STARK_TRANSITION) a = gl_mul(a, z_last);
            else if (slot == GL_STARK_FIRST_ROW) a = gl_mul(a, lf);
            else if (slot == GL_STARK_LAST_ROW) a = gl_mul(a, ll);
            GLS_CONSUME(a);
            continue;
        }
        GLS_OPERAND(b, w.z);
        mine[slot * GLS_DAG_BLOCK] = op == GL_STARK_OP_MUL ? gl_mul(a, b) : op == GL_STARK_OP_ADD ? gl_add(a, b) : gl_sub(a, b);
    }
#undef GLS_OPERAND
    // eval_permutation_checks (permutation.rs:282-320), as in k_stark_quotient
    for (uint32_t b = 0; b < p.nz; b++) GLS_CONSUME(gl_mul(gl_sub(p.zs[(size_t)b * p.stride + il], 1), lf));
    for (uint32_t b = 0; b < p.nz; b++) {
        const uint32_t e0 = b * p.q, e1 = min(e0 + p.q, p.num_instances);
        gl_t pl = p.zs[(size_t)b * p.stride + il], pr = p.zs[(size_t)b * p.stride + in];
        for (uint32_t e = e0; e < e1; e++) {
            const uint32_t pair = e / p.nc, chal = e % p.nc, j = e - e0;
            const gl_t beta = p.ch[(j * p.nc + chal) * 2], gamma = p.ch[(j * p.nc + chal) * 2 + 1];
            const uint32_t off = p.pair_off[pair], len = p.pair_off[pair + 1] - off;
            gl_t lhs = 0, rhs = 0;
            for (uint32_t k = len; k-- > 0;) {
                lhs = gl_mul_add(p.trace[(size_t)p.pair_cols[2 * (off + k)] * p.stride + il], lhs, beta);
                rhs = gl_mul_add(p.trace[(size_t)p.pair_cols[2 * (off + k) + 1] * p.stride + il], rhs, beta);
            }
            pl = gl_mul(pl, gl_add_c(lhs, gamma));
            pr = gl_mul(pr, gl_add_c(rhs, gamma));
        }
        GLS_CONSUME(gl_sub(pr, pl));
    }
#undef GLS_CONSUME
    const gl_t zi = p.zh_inv[i & (p.next_step - 1)];
    p.out[i] = gl_canon(gl_mul(a0, zi));
    if (NC > 1) p.out[(size_t)p.size + i] = gl_canon(gl_mul(a1, zi));
    if (NC > 2) p.out[(size_t)2 * p.size + i] = gl_canon(gl_mul(a2, zi));
    if (NC > 3) p.out[(size_t)3 * p.size + i] = gl_canon(gl_mul(a3, zi));
}
