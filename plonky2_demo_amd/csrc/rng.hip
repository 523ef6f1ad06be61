// Randomness of zero-knowledge proving on the device: the keystream of rng.cuh written straight into HBM (salt columns of a
// PolynomialBatch, blinding rows of a witness), and the OS seed.
#include "context.hpp"
#include "rng.cuh"
#include <sys/random.h>
#include <errno.h>

int gl_os_seed(uint8_t seed[32]) {
    size_t got = 0;
    while (got < 32) {
        const ssize_t r = getrandom(seed + got, 32 - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return gl_fail(GL_ERR_INTERNAL, "getrandom(2) failed", __FILE__, __LINE__);
        }
        got += (size_t)r;
    }
    return GL_OK;
}

// one thread per keystream block (4 elements); blockIdx.y = stream offset
__global__ void k_random_elements(gl_chacha_key key, uint32_t stream0, uint64_t first, uint64_t count, gl_t* out, uint64_t out_stride) {
    const uint64_t blk = (first >> 2) + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t lo = blk << 2, end = first + count;
    if (lo >= end) return;
    const uint32_t stream = stream0 + blockIdx.y;
    uint32_t ks[16];
    gl_chacha20_block(key, stream, (uint32_t)blk, ks);
    gl_t* o = out + (uint64_t)blockIdx.y * out_stride;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t i = lo + j;
        if (i >= first && i < end) o[i - first] = gl_chacha_element(ks, j);
    }
}

int gl_fill_random(gl_ctx* c, const uint8_t seed[32], uint32_t stream0, uint32_t nstreams, uint64_t first, uint64_t count, gl_t* d_out,
                   uint64_t out_stride) {
    GL_REQUIRE(seed && d_out && nstreams >= 1 && nstreams <= 65535, GL_ERR_ARG, "random elements: bad argument");
    GL_REQUIRE(first + count >= first && first + count <= (uint64_t(1) << 34), GL_ERR_ARG, "random elements: index beyond 2^34 (32-bit block counter)");
    if (!count) return GL_OK;
    const uint64_t blocks = ((first + count + 3) >> 2) - (first >> 2);
    hipLaunchKernelGGL(k_random_elements, dim3((unsigned)((blocks + 255) / 256), nstreams), dim3(256), 0, c->stream, gl_chacha_key_from_bytes(seed),
                       stream0, first, count, d_out, out_stride);
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}

extern "C" int gl_random_elements(gl_ctx* c, const uint8_t seed[32], uint32_t stream, uint64_t first, uint64_t count, uint64_t* d_out) try {
    GL_REQUIRE(c && seed && d_out, GL_ERR_ARG, "gl_random_elements: null argument");
    GL_TRY(c->activate());
    return gl_fill_random(c, seed, stream, 1, first, count, d_out, 0);
} catch (...) { return gl_caught(); }

// RandomValueGenerator + CopyGenerator of blind() (circuit_builder.rs:777-818), then full_witness's zeros (iop/witness.rs:340-352):
// rows g .. g + regular: all 135 wires random; then `pairs` row pairs whose first row's 80 routed wires are random and copied to the
// second row, the rest 0; the padding rows after them 0.  One thread per (row, wire), row >= g.
__global__ void k_witness_blind(gl_chacha_key key, gl_t* wires, uint32_t n, uint32_t g, uint32_t regular, uint32_t pairs) {
    const uint32_t row = g + blockIdx.x * blockDim.x + threadIdx.x, w = blockIdx.y;
    if (row >= n) return;
    const uint32_t r = row - g;
    gl_t v = 0;
    if (r < regular) v = gl_random_element(key, GL_STREAM_WIRE + w, row);
    else if (r - regular < 2 * pairs && w < 80) v = gl_random_element(key, GL_STREAM_WIRE + w, row - ((r - regular) & 1));
    wires[(uint64_t)w * n + row] = v;
}

int gl_launch_witness_blind(gl_ctx* c, const uint8_t seed[32], gl_t* d_wires, uint32_t n, uint32_t g, uint32_t regular, uint32_t pairs) {
    GL_REQUIRE(seed && d_wires && g <= n && (uint64_t)g + regular + 2ull * pairs <= n, GL_ERR_ARG, "gl_witness_blind: blinding rows do not fit");
    if (g == n) return GL_OK;
    hipLaunchKernelGGL(k_witness_blind, dim3((n - g + 255) / 256, 135), dim3(256), 0, c->stream, gl_chacha_key_from_bytes(seed), d_wires, n, g,
                       regular, pairs);
    GL_CHECK_HIP(hipGetLastError());
    return GL_OK;
}
