// Device kernels of the STARK prover (starky/src): the two phases between the polynomial commitments that the Plonk path has no
// counterpart for, with the AIR handed over as data (gl_stark_desc, include/plonky2_mi355x.h).
//   k_stark_perm_quotients / k_stark_seg_* / k_stark_z_finalize   permutation-argument Z polynomials (permutation.rs:66-117)
//   k_stark_lagrange_on_coset                                     L_first, L_last on the quotient coset (prover.rs:230-234), once per gl_stark
//   k_stark_quotient                                              sum_i alpha^i C_i(x) / Z_H(x) on the quotient coset (prover.rs:198-318,
//                                                                 constraint_consumer.rs:33-77, permutation.rs:262-321)
//   k_stark_tail_nonzero                                          the trim_to_len check of prover.rs:123-128
// The term program and the pair tables are read through kernel arguments and loop counters only: every address is wave-uniform, the
// loads are scalar and every branch on the program is uniform.  All values are exact field elements.
#pragma once
#include "gl64.cuh"
#include "stark_segments.cuh"
#include "../../include/plonky2_mi355x.h"

struct GlStarkPerm {
    const gl_t* trace;          // trace VALUES [num_columns][n]
    const gl_t* ch;             // [q][num_challenges][2] (beta, gamma), canonical
    const uint32_t* pair_off;   // [num_pairs + 1] start of each pair in pair_cols (in column pairs)
    const uint32_t* pair_cols;  // [sum pair_len][2] (lhs, rhs)
    uint32_t n, q, nc, num_instances;
};

// quotient[b][i] = prod_inst (gamma + sum_k beta^k lhs_k(i)) / prod_inst (gamma + sum_k beta^k rhs_k(i)) over the instances of Z
// polynomial b = blockIdx.y: instance j of the batch is (pair, chal) number b q + j of pairs x 0..num_challenges and takes
// challenge_sets[j].challenges[chal] (get_permutation_batches, permutation.rs:228-249).  A thread owns GLS_ROWS rows, 256 apart.
__global__ __launch_bounds__(256) void k_stark_perm_quotients(GlStarkPerm p, gl_t* __restrict__ quot /* [nz][n] */, uint32_t* zero_flag) {
    const uint32_t b = blockIdx.y, base = blockIdx.x * GLS_SEG + threadIdx.x;
    const uint32_t e0 = b * p.q, e1 = min(e0 + p.q, p.num_instances);
    gl_t num[GLS_ROWS], den[GLS_ROWS];
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) { num[r] = 1; den[r] = 1; }
    for (uint32_t e = e0; e < e1; e++) {
        const uint32_t pair = e / p.nc, chal = e % p.nc, j = e - e0;
        const gl_t beta = p.ch[(j * p.nc + chal) * 2], gamma = p.ch[(j * p.nc + chal) * 2 + 1];
        const uint32_t off = p.pair_off[pair], len = p.pair_off[pair + 1] - off;
#pragma unroll
        for (int r = 0; r < GLS_ROWS; r++) {
            const uint32_t i = base + r * 256;
            if (i >= p.n) continue;
            gl_t lhs = 0, rhs = 0;                          // Horner from the last column pair: sum_k beta^k col_k
            for (uint32_t k = len; k-- > 0;) {
                lhs = gl_mul_add(p.trace[(size_t)p.pair_cols[2 * (off + k)] * p.n + i], lhs, beta);
                rhs = gl_mul_add(p.trace[(size_t)p.pair_cols[2 * (off + k) + 1] * p.n + i], rhs, beta);
            }
            num[r] = gl_mul(num[r], gl_add_c(lhs, gamma));
            den[r] = gl_mul(den[r], gl_add_c(rhs, gamma));
        }
    }
    gl_t pre[GLS_ROWS], acc = 1;
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) { pre[r] = acc; acc = gl_mul(acc, den[r]); }
    if (gl_canon(acc) == 0) atomicOr(zero_flag, 1u);         // the reference panics in batch_multiplicative_inverse
    gl_t inv = gl_inv(acc);
#pragma unroll
    for (int r = GLS_ROWS - 1; r >= 0; r--) {
        const uint32_t i = base + r * 256;
        const gl_t dinv = gl_mul(inv, pre[r]);
        inv = gl_mul(inv, den[r]);
        if (i < p.n) quot[(size_t)b * p.n + i] = gl_canon(gl_mul(num[r], dinv));
    }
}

// ---- exclusive multiplicative scan over rows, Z[i] = prod_{i' < i} quotient[i'] (the three-launch shape of prover_kernels.cuh's
//      k_z_segment_products / k_z_segment_scan / k_z_finalize, for any number of polynomials) ----
__global__ __launch_bounds__(256) void k_stark_seg_products(const gl_t* quot, uint32_t n, gl_t* seg_prod) {
    __shared__ gl_t sh[256];
    const uint32_t b = blockIdx.y, seg = blockIdx.x, t = threadIdx.x;
    const gl_t* rp = quot + (size_t)b * n;
    gl_t acc = 1;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLS_SEG + t * 8 + q; if (i < n) acc = gl_mul(acc, rp[i]); }
    sh[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (t < s) sh[t] = gl_mul(sh[t], sh[t + s]); __syncthreads(); }
    if (t == 0) seg_prod[(size_t)b * gridDim.x + seg] = gl_canon(sh[0]);
}
// one thread per polynomial; segment counts are tiny
__global__ void k_stark_seg_scan(gl_t* seg_prod, uint32_t nseg, uint32_t nz) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nz) return;
    gl_t acc = 1;
    for (uint32_t s = 0; s < nseg; s++) { const gl_t v = seg_prod[(size_t)b * nseg + s]; seg_prod[(size_t)b * nseg + s] = acc; acc = gl_canon(gl_mul(acc, v)); }
}
__global__ __launch_bounds__(256) void k_stark_z_finalize(const gl_t* quot, const gl_t* seg_excl, uint32_t n, gl_t* __restrict__ out /* [nz][n] */) {
    __shared__ gl_t sh[256];
    const uint32_t b = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, nseg = gridDim.x;
    const gl_t* rp = quot + (size_t)b * n;
    gl_t loc[8];
    gl_t acc = 1;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLS_SEG + t * 8 + q; loc[q] = acc; if (i < n) acc = gl_mul(acc, rp[i]); }
    sh[t] = acc;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                      // Hillis-Steele on the 256 per-thread products
        const gl_t v = (t >= (uint32_t)d) ? sh[t - d] : 1;
        __syncthreads();
        sh[t] = gl_mul(sh[t], v);
        __syncthreads();
    }
    const gl_t prefix = gl_mul(seg_excl[(size_t)b * nseg + seg], t ? sh[t - 1] : 1);
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint32_t i = seg * GLS_SEG + t * 8 + q;
        if (i < n) out[(size_t)b * n + i] = gl_canon(gl_mul(prefix, loc[q]));
    }
}

// L_first(x) = Z_H(x) / (n (x - 1)) and L_last(x) = Z_H(x) g^-1 / (n (x - g^-1)) at x_i = 7 w^i, i < size: value for value the
// reference's selector(degree, 0 | degree - 1).lde_onto_coset (prover.rs:230-234).  One inversion per point serves both; the tables
// are built once per gl_stark, not per proof.  zh[i mod 2^qdb] = Z_H(x_i).
__global__ __launch_bounds__(256) void k_stark_lagrange_on_coset(const gl_t* xpow_lo, const gl_t* xpow_hi, uint32_t size, uint32_t zh_mask, const gl_t* zh,
                                                                 gl_t n_inv, gl_t last, gl_t* lfirst, gl_t* llast) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= size) return;
    const gl_t x = gl_mul(xpow_lo[i & 2047], xpow_hi[i >> 11]);
    const gl_t a = gl_sub(x, 1), c = gl_sub(x, last);
    const gl_t inv = gl_inv(gl_mul(a, c));                  // x is off H: neither factor is zero
    const gl_t zn = gl_mul(zh[i & zh_mask], n_inv);
    lfirst[i] = gl_canon(gl_mul(zn, gl_mul(inv, c)));
    llast[i] = gl_canon(gl_mul(gl_mul(zn, last), gl_mul(inv, a)));
}

struct GlStarkQuot {
    const gl_t* trace;          // trace LDE [num_columns][stride], natural order
    const gl_t* zs;             // Z LDE [nz][stride], or null without pairs
    uint64_t stride;            // n << rate_bits
    // the term program (gl_stark_desc), device copies
    const uint32_t* filter; const uint32_t* num_terms; const uint32_t* term_nf; const uint32_t* factors;
    const gl_t* coeff;          // canonical
    const gl_t* pub;            // [num_public_inputs] canonical
    const gl_t* ch;             // [q][num_challenges][2], canonical
    const uint32_t* pair_off; const uint32_t* pair_cols;
    const gl_t* xpow_lo; const gl_t* xpow_hi;   // 7 w_size^i two-level
    const gl_t* lfirst; const gl_t* llast;      // [size]
    gl_t* out;                  // [num_challenges][size]
    gl_t alphas[4];
    gl_t zh_inv[8];             // 1 / Z_H(x_i) by i mod 2^qdb (ZeroPolyOnCoset::eval_inverse)
    gl_t last;                  // g^-1, the last element of H
    uint32_t size, step, next_step, num_constraints, nc, q, nz, num_instances;
};

// One thread per point i of the quotient coset.  local = lde[col][i step], next = lde[col][((i + 2^qdb) mod size) step].
template <int NC>
__global__ __launch_bounds__(256) void k_stark_quotient(GlStarkQuot p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.size) return;
    const size_t il = (size_t)i * p.step, in = (size_t)((i + p.next_step) & (p.size - 1)) * p.step;
    const gl_t x = gl_mul(p.xpow_lo[i & 2047], p.xpow_hi[i >> 11]);
    const gl_t z_last = gl_sub(x, p.last), lf = p.lfirst[i], ll = p.llast[i];
    gl_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;                    // ConstraintConsumer::constraint_accs, one register pair each
#define GLS_CONSUME(C)                                                  \
    do {                                                                \
        const gl_t _c = (C);                                            \
        a0 = gl_mul_add(_c, a0, p.alphas[0]);                           \
        if (NC > 1) a1 = gl_mul_add(_c, a1, p.alphas[1]);               \
        if (NC > 2) a2 = gl_mul_add(_c, a2, p.alphas[2]);               \
        if (NC > 3) a3 = gl_mul_add(_c, a3, p.alphas[3]);               \
    } while (0)
    // the Stark's own constraints: C = sum_t coeff_t prod_f operand_{t,f}, then the filter (constraint_consumer.rs:53-76)
    uint32_t t = 0, f = 0;
    for (uint32_t c = 0; c < p.num_constraints; c++) {
        gl_t C = 0;
        const uint32_t t_end = t + p.num_terms[c];
        for (; t < t_end; t++) {
            gl_t m = p.coeff[t];
            const uint32_t f_end = f + p.term_nf[t];
            for (; f < f_end; f++) {
                const uint32_t w = p.factors[f], kind = w >> 30, idx = w & 0x3FFFFFFFu;
                gl_t v;
                if (kind == GL_STARK_LOCAL) v = p.trace[(size_t)idx * p.stride + il];
                else if (kind == GL_STARK_NEXT) v = p.trace[(size_t)idx * p.stride + in];
                else v = p.pub[idx];
                m = gl_mul(m, v);
            }
            C = gl_add(C, m);
        }
        const uint32_t filt = p.filter[c];
        if (filt == GL_STARK_TRANSITION) C = gl_mul(C, z_last);
        else if (filt == GL_STARK_FIRST_ROW) C = gl_mul(C, lf);
        else if (filt == GL_STARK_LAST_ROW) C = gl_mul(C, ll);
        GLS_CONSUME(C);
    }
    // eval_permutation_checks (permutation.rs:282-320): Z_b - 1 on the first row for every b, then per b
    // Z_b(next) prod rhs - Z_b(local) prod lhs on all rows
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

// trim_to_len (prover.rs:123-128): the coefficients from index `from` on of each of `count` polynomials of `size` must be zero
__global__ __launch_bounds__(256) void k_stark_tail_nonzero(const gl_t* coeffs, uint32_t size, uint32_t from, uint32_t* flag) {
    const uint32_t i = from + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < size && gl_canon(coeffs[(size_t)blockIdx.y * size + i]) != 0) atomicOr(flag, 1u);
}
