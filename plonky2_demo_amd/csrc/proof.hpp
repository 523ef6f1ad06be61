// The proof handle of the C ABI: prove.hip fills it, host_api.hip reads it back out.
#pragma once
#include <stdint.h>
#include <vector>
#include "gl64.cuh"

struct gl_proof {
    std::vector<uint8_t> bytes;
    std::vector<gl_t> challenges;     // betas gammas alphas zeta fri_alpha pow pi_hash fri_betas...
    std::vector<gl_t> caps;           // 3 x 16 x 4
    std::vector<gl_t> zs_pp;          // [20][n]
    std::vector<gl_t> quotient;       // [16][n]
    std::vector<uint64_t> query_indices;
};
