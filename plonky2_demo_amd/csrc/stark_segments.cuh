// The row tiling that the running-product kernels of stark_kernels.cuh and stark_ctl_kernels.cuh share: seg_products_scan (stark.hip) and
// both finalize kernels must agree on it.
#pragma once
#define GLS_SEG 2048            // rows per workgroup segment of the scan (256 threads x 8)
#define GLS_ROWS 8              // rows per thread of k_stark_perm_quotients (one inversion for 8 denominators) and of k_stark_ctl_factors
