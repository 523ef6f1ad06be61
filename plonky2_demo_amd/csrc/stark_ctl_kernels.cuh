// Device kernels of cross-table lookups between STARK tables (evm/src/cross_table_lookup.rs), the lookups handed over as data
// (gl_stark_set_desc, include/plonky2_mi355x.h):
//   k_stark_ctl_factors             the per-row factors of the CTL running products (partial_products, :279-306)
//   k_stark_z_finalize_inclusive    the inclusive sibling of stark_kernels.cuh's k_stark_z_finalize; the segment products and their scan are
//                                   that file's k_stark_seg_products / k_stark_seg_scan, launched by stark.hip
//   k_stark_quotient_ctl            the two CTL checks per Z (:374-414), folded into the values k_stark_quotient left
// They stand in a file and a translation unit of their own (stark_set.hip), so that the single-table kernels' code objects stay as they
// are.  The Column program is read through kernel arguments and loop counters only: scalar loads, uniform branches; the filter select is
// per lane.  All values are exact field elements.
#pragma once
#include "gl64.cuh"
#include "stark_segments.cuh"
#include "../../include/plonky2_mi355x.h"

// ---- the running products of evm/src/cross_table_lookup.rs:279-306 (partial_products) ----
struct GlStarkCtl {
    const gl_t* trace;          // trace VALUES [num_columns][n]
    const gl_t* ch;             // [num_challenges][2] (beta, gamma), canonical
    const uint32_t* z_prog;     // [nzc][4]: first Column, number of Columns, 1 = a filter Column follows them, challenge index
    const uint32_t* col_off;    // [Columns + 1] start of each Column's terms
    const uint32_t* term_col;   // [terms] trace column
    const gl_t* term_coeff;     // [terms] canonical
    const gl_t* col_const;      // [Columns] canonical
    uint32_t n;
};

// Column::eval_table (cross_table_lookup.rs:110-116) of Column c on the GLS_ROWS rows of a thread: constant + sum coeff * trace[column].
// The term list is reached through the kernel argument and the loop counter: scalar loads, uniform branches.  Rows past n read nothing.
__device__ __forceinline__ void gls_ctl_column(const GlStarkCtl& p, uint32_t c, uint32_t base, gl_t (&v)[GLS_ROWS]) {
    const gl_t k = p.col_const[c];
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) v[r] = k;
    const uint32_t t_end = p.col_off[c + 1];
    for (uint32_t t = p.col_off[c]; t < t_end; t++) {
        const gl_t* col = p.trace + (size_t)p.term_col[t] * p.n;
        const gl_t w = p.term_coeff[t];
        if (w == 1) {                                       // Column::single / ::sum: no product
#pragma unroll
            for (int r = 0; r < GLS_ROWS; r++) { const uint32_t i = base + r * 256; if (i < p.n) v[r] = gl_add(v[r], col[i]); }
        } else {
#pragma unroll
            for (int r = 0; r < GLS_ROWS; r++) { const uint32_t i = base + r * 256; if (i < p.n) v[r] = gl_mul_add(v[r], col[i], w); }
        }
    }
}

// factor[b][i] of CTL Z b = blockIdx.y: combine(columns(row i)) = gamma + sum_k beta^k Column_k(row i) where the filter Column is 1 (or
// there is none), 1 where it is 0; another filter value raises the flag and leaves 1.  The filter select is per lane.  A thread owns
// GLS_ROWS rows, 256 apart, as in k_stark_perm_quotients.
__global__ __launch_bounds__(256) void k_stark_ctl_factors(GlStarkCtl p, gl_t* __restrict__ fac /* [nzc][n] */, uint32_t* bad_filter) {
    const uint32_t b = blockIdx.y, base = blockIdx.x * GLS_SEG + threadIdx.x;
    const uint32_t c0 = p.z_prog[4 * b], ncols = p.z_prog[4 * b + 1], has_filter = p.z_prog[4 * b + 2], chal = p.z_prog[4 * b + 3];
    const gl_t beta = p.ch[2 * chal], gamma = p.ch[2 * chal + 1];
    gl_t acc[GLS_ROWS], v[GLS_ROWS];
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) acc[r] = 0;
    for (uint32_t k = ncols; k-- > 0;) {                    // Horner from the last Column: sum_k beta^k Column_k
        gls_ctl_column(p, c0 + k, base, v);
#pragma unroll
        for (int r = 0; r < GLS_ROWS; r++) acc[r] = gl_mul_add(v[r], acc[r], beta);
    }
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) acc[r] = gl_add_c(acc[r], gamma);
    if (has_filter) {
        gls_ctl_column(p, c0 + ncols, base, v);
        bool bad = false;
#pragma unroll
        for (int r = 0; r < GLS_ROWS; r++) {
            const gl_t f = gl_canon(v[r]);
            acc[r] = f == 1 ? acc[r] : 1;
            bad |= f > 1 && base + r * 256 < p.n;
        }
        if (bad) atomicOr(bad_filter, 1u);                   // the reference asserts "Non-binary filter?"
    }
#pragma unroll
    for (int r = 0; r < GLS_ROWS; r++) {
        const uint32_t i = base + r * 256;
        if (i < p.n) fac[(size_t)b * p.n + i] = gl_canon(acc[r]);
    }
}

// k_stark_z_finalize's inclusive sibling, Z[i] = prod_{i' <= i} factor[i']: the same segment prefixes, each row's own factor multiplied in
__global__ __launch_bounds__(256) void k_stark_z_finalize_inclusive(const gl_t* fac, const gl_t* seg_excl, uint32_t n, gl_t* __restrict__ out /* [nz][n] */) {
    __shared__ gl_t sh[256];
    const uint32_t b = blockIdx.y, seg = blockIdx.x, t = threadIdx.x, nseg = gridDim.x;
    const gl_t* rp = fac + (size_t)b * n;
    gl_t loc[8];
    gl_t acc = 1;
#pragma unroll
    for (int q = 0; q < 8; q++) { const uint32_t i = seg * GLS_SEG + t * 8 + q; if (i < n) acc = gl_mul(acc, rp[i]); loc[q] = acc; }
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

// eval_cross_table_lookup_checks (cross_table_lookup.rs:374-414) as a pass of its own AFTER k_stark_quotient, whose code stays as it is.
// The consumer is Horner in alpha, so m further constraints turn  out = acc Z_H^-1  into  out alpha^m + acc' Z_H^-1  with acc' the Horner
// sum of the m new ones alone: exact field arithmetic, the same words a fused kernel gives.  Per CTL Z b, in order:
//   first row   Z(x) - select(f(x), combine(x))                 select(f, c) = f c + 1 - f
//   transition  Z(g x) - Z(x) select(f(g x), combine(g x))
struct GlStarkQuotCtl {
    GlStarkCtl c;               // c.trace = trace LDE [num_columns][stride]; c.ch the CTL challenges; c.n unused
    const gl_t* zs;             // LDE of the table's first CTL Z: [nctl][stride] (the permutation Zs stand before it)
    uint64_t stride;
    const gl_t* xpow_lo; const gl_t* xpow_hi; const gl_t* lfirst;
    gl_t* out;                  // [num_challenges][size], read and written
    gl_t alphas[4], alpha_pow[4];   // alpha_j and alpha_j^(2 nctl)
    gl_t zh_inv[8];
    gl_t last;
    uint32_t size, step, next_step, nctl;
};

// Column c on the local and the next row of one point
__device__ __forceinline__ void gls_ctl_column_pair(const GlStarkCtl& p, uint32_t c, uint64_t stride, size_t il, size_t in, gl_t& vl, gl_t& vn) {
    vl = vn = p.col_const[c];
    const uint32_t t_end = p.col_off[c + 1];
    for (uint32_t t = p.col_off[c]; t < t_end; t++) {
        const gl_t* col = p.trace + (size_t)p.term_col[t] * stride;
        const gl_t w = p.term_coeff[t];
        if (w == 1) {                                       // Column::single / ::sum: no product (a uniform branch)
            vl = gl_add(vl, col[il]);
            vn = gl_add(vn, col[in]);
        } else {
            vl = gl_mul_add(vl, col[il], w);
            vn = gl_mul_add(vn, col[in], w);
        }
    }
}

template <int NC>
__global__ __launch_bounds__(256) void k_stark_quotient_ctl(GlStarkQuotCtl p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.size) return;
    const size_t il = (size_t)i * p.step, in = (size_t)((i + p.next_step) & (p.size - 1)) * p.step;
    const gl_t x = gl_mul(p.xpow_lo[i & 2047], p.xpow_hi[i >> 11]);
    const gl_t z_last = gl_sub(x, p.last), lf = p.lfirst[i];
    gl_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#define GLS_CONSUME(C)                                                  \
    do {                                                                \
        const gl_t _c = (C);                                            \
        a0 = gl_mul_add(_c, a0, p.alphas[0]);                           \
        if (NC > 1) a1 = gl_mul_add(_c, a1, p.alphas[1]);               \
        if (NC > 2) a2 = gl_mul_add(_c, a2, p.alphas[2]);               \
        if (NC > 3) a3 = gl_mul_add(_c, a3, p.alphas[3]);               \
    } while (0)
    for (uint32_t b = 0; b < p.nctl; b++) {
        const uint32_t c0 = p.c.z_prog[4 * b], ncols = p.c.z_prog[4 * b + 1], has_filter = p.c.z_prog[4 * b + 2], chal = p.c.z_prog[4 * b + 3];
        const gl_t beta = p.c.ch[2 * chal], gamma = p.c.ch[2 * chal + 1];
        gl_t cl = 0, cn = 0, vl, vn;
        for (uint32_t k = ncols; k-- > 0;) {
            gls_ctl_column_pair(p.c, c0 + k, p.stride, il, in, vl, vn);
            cl = gl_mul_add(vl, cl, beta);
            cn = gl_mul_add(vn, cn, beta);
        }
        cl = gl_add_c(cl, gamma);
        cn = gl_add_c(cn, gamma);
        if (has_filter) {                                   // select(f, c) = f (c - 1) + 1
            gls_ctl_column_pair(p.c, c0 + ncols, p.stride, il, in, vl, vn);
            cl = gl_mul_add(1, vl, gl_sub(cl, 1));
            cn = gl_mul_add(1, vn, gl_sub(cn, 1));
        }
        const gl_t zl = p.zs[(size_t)b * p.stride + il], zn = p.zs[(size_t)b * p.stride + in];
        GLS_CONSUME(gl_mul(gl_sub(zl, cl), lf));
        GLS_CONSUME(gl_mul(gl_sub(zn, gl_mul(zl, cn)), z_last));
    }
#undef GLS_CONSUME
    const gl_t zi = p.zh_inv[i & (p.next_step - 1)];
    p.out[i] = gl_canon(gl_mul_add(gl_mul(a0, zi), p.out[i], p.alpha_pow[0]));
    if (NC > 1) p.out[(size_t)p.size + i] = gl_canon(gl_mul_add(gl_mul(a1, zi), p.out[(size_t)p.size + i], p.alpha_pow[1]));
    if (NC > 2) p.out[(size_t)2 * p.size + i] = gl_canon(gl_mul_add(gl_mul(a2, zi), p.out[(size_t)2 * p.size + i], p.alpha_pow[2]));
    if (NC > 3) p.out[(size_t)3 * p.size + i] = gl_canon(gl_mul_add(gl_mul(a3, zi), p.out[(size_t)3 * p.size + i], p.alpha_pow[3]));
}
