// The reference's test_fibonacci_stark (starky/src/fibonacci_stark.rs:137-158) over the C ABI: the Fibonacci AIR as a term list, a trace
// of 2^5 rows from x0 = 0, x1 = 1, prove, print the sizes, verify.
//
//   fibonacci_stark [log2 of the rows = 5] [--keccak]
//
// Plain C++ over include/plonky2_mi355x.h; the only GPU-specific line is gl_ctx_create.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/plonky2_mi355x.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int _st = (call);                                                            \
        if (_st != GL_OK) { fprintf(stderr, "%s failed (%d): %s\n", #call, _st, gl_last_error()); return 1; } \
    } while (0)

static const uint64_t P = 0xFFFFFFFF00000001ULL;
static uint64_t add(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % P); }
static uint32_t local(uint32_t c) { return GL_STARK_LOCAL << 30 | c; }
static uint32_t next(uint32_t c) { return GL_STARK_NEXT << 30 | c; }
static uint32_t pub(uint32_t i) { return GL_STARK_PUBLIC << 30 | i; }

int main(int argc, char** argv) {
    bool keccak = false;
    unsigned degree_bits = 5;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--keccak")) keccak = true;
        else degree_bits = (unsigned)atoi(argv[i]);
    }
    if (degree_bits < 1 || degree_bits > 20) { fprintf(stderr, "1 <= log2 of the rows <= 20\n"); return 1; }
    const size_t n = size_t(1) << degree_bits;

    // ---- FibonacciStark::eval_packed_generic (fibonacci_stark.rs:64-86) as data: columns x0, x1, i, j; public inputs x0, x1, result ----
    const uint64_t one = 1, minus_one = P - 1;
    const uint32_t filter[5] = {GL_STARK_FIRST_ROW, GL_STARK_FIRST_ROW, GL_STARK_LAST_ROW, GL_STARK_TRANSITION, GL_STARK_TRANSITION};
    const uint32_t num_terms[5] = {2, 2, 2, 2, 3};
    const uint64_t coeff[11] = {one, minus_one, one, minus_one, one, minus_one, one, minus_one, one, minus_one, minus_one};
    const uint32_t num_factors[11] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    const uint32_t factors[11] = {local(0), pub(0),             // local[0] - x0        on the first row
                                  local(1), pub(1),             // local[1] - x1        on the first row
                                  local(1), pub(2),             // local[1] - result    on the last row
                                  next(0), local(1),            // next[0] - local[1]   on transitions
                                  next(1), local(0), local(1)}; // next[1] - local[0] - local[1]
    const uint32_t pair_len[1] = {1}, pair_columns[2] = {2, 3};  // permutation_pairs(): columns 2 and 3 hold the same values
    gl_stark_desc desc;
    memset(&desc, 0, sizeof desc);
    desc.num_columns = 4; desc.num_public_inputs = 3; desc.constraint_degree = 2;
    desc.num_challenges = 2;                                     // StarkConfig::standard_fast_config (starky/src/config.rs:17-29)
    desc.num_constraints = 5;
    desc.constraint_filter = filter; desc.constraint_num_terms = num_terms; desc.term_coeff = coeff; desc.term_num_factors = num_factors; desc.factors = factors;
    desc.num_permutation_pairs = 1; desc.pair_len = pair_len; desc.pair_columns = pair_columns;
    gl_fri_params params;
    memset(&params, 0, sizeof params);
    params.degree_bits = degree_bits; params.rate_bits = 1; params.cap_height = 4; params.proof_of_work_bits = 16; params.num_query_rounds = 84;
    for (unsigned left = degree_bits; left > 5 && left + 1 - 4 >= 4; left -= 4) params.fri_arity_bits[params.num_fri_rounds++] = 4;      // ConstantArityBits(4, 5)
    params.hasher = keccak ? GL_HASHER_KECCAK : GL_HASHER_POSEIDON;
    CHECK(gl_stark_check(&desc, &params));

    // ---- generate_trace (fibonacci_stark.rs:44-57) ----
    std::vector<std::vector<uint64_t>> cols(4, std::vector<uint64_t>(n));
    uint64_t row[4] = {0, 1, 0, 1};
    for (size_t i = 0; i < n; i++) {
        for (int c = 0; c < 4; c++) cols[c][i] = row[c];
        const uint64_t x0 = row[0];
        row[0] = row[1]; row[1] = add(x0, row[1]); row[2] = add(row[2], 1); row[3] = add(row[3], 1);
    }
    cols[3][n - 1] = 0;                                          // so that columns 2 and 3 are permutations of one another
    const uint64_t public_inputs[3] = {0, 1, cols[1][n - 1]};
    const uint64_t* col_ptrs[4] = {cols[0].data(), cols[1].data(), cols[2].data(), cols[3].data()};

    // ---- prove ----
    gl_ctx* ctx = nullptr;
    CHECK(gl_ctx_create(0, nullptr, &ctx));
    gl_stark* stark = nullptr;
    CHECK(gl_stark_create(ctx, &desc, &params, &stark));
    std::vector<uint8_t> proof(gl_stark_proof_size(stark));
    size_t num_bytes = 0;
    CHECK(gl_stark_prove(ctx, stark, col_ptrs, public_inputs, proof.data(), proof.size(), &num_bytes));
    printf("fibonacci: %zu rows, result %llu, %u FRI reductions, proof %zu bytes (%s)\n", n, (unsigned long long)public_inputs[2], params.num_fri_rounds,
           num_bytes, keccak ? "Keccak" : "Poseidon");

    // ---- verify: host code, needs only the description, the params and the bytes ----
    uint32_t check = 0;
    CHECK(gl_stark_verify(&desc, &params, proof.data(), num_bytes, &check));
    printf("verified\n");
    proof[num_bytes - 8] ^= 1;                                   // another result than the trace's
    if (gl_stark_verify(&desc, &params, proof.data(), num_bytes, &check) != GL_ERR_VERIFY || check != GL_CHECK_VANISHING) {
        fprintf(stderr, "a proof with a changed public input was not rejected\n");
        return 1;
    }
    printf("a changed public input is rejected: %s\n", gl_last_error());
    gl_stark_free(stark);
    gl_ctx_destroy(ctx);
    return 0;
}
