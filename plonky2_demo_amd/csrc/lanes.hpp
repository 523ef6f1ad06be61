// The lane runner of the prover pools (witness.hip): `count` items fanned out over `lanes` host threads inside one call.  No
// kernels and no HIP calls here, so tools/sanitizer/abi_unwind.cpp runs it on the CPU with failing allocations.
//   * item i goes to lane i % lanes; lane 0 runs on the calling thread;
//   * `work(lane, i)` returns a status and leaves its text in its own thread's last error; an exception it throws becomes
//     GL_ERR_INTERNAL for that lane (in a worker thread it would otherwise be std::terminate);
//   * lanes stop taking items once any lane has failed; the call returns the FIRST failing status with that lane's text;
//   * a thread that cannot be started is such a failure: no further thread is started, lane 0 still runs (and returns at
//     once), and every thread that was started is joined.
#pragma once
#include "context.hpp"
#include <atomic>
#include <cstring>
#include <thread>

constexpr size_t GL_MAX_LANES = 64;

template <class Work>
int gl_run_lanes(size_t lanes, size_t count, const char* who, Work&& work) noexcept {
    GL_REQUIRE(lanes >= 1 && lanes <= GL_MAX_LANES, GL_ERR_INTERNAL, "lane count out of range");
    std::atomic<int> first_error{GL_OK};
    char message[sizeof g_gl_last_error] = "";      // written by the one lane that sets first_error, read after the joins
    auto fail = [&](int st) noexcept {
        int expected = GL_OK;
        if (first_error.compare_exchange_strong(expected, st)) { strncpy(message, g_gl_last_error, sizeof message - 1); }
    };
    auto run = [&](size_t lane) noexcept {
        for (size_t i = lane; i < count && first_error.load() == GL_OK; i += lanes) {
            int st;
            try { st = work(lane, i); } catch (...) { st = gl_caught(); }
            if (st != GL_OK) fail(st);
        }
    };
    std::thread threads[GL_MAX_LANES];               // (not a vector: growing one can throw with joinable threads inside)
    size_t started = 0;
    for (size_t k = 1; k < lanes && k < count; k++) {
        try { threads[k] = std::thread(run, k); started = k; }
        catch (...) { fail(gl_caught()); break; }
    }
    run(0);
    for (size_t k = 1; k <= started; k++) threads[k].join();
    const int st = first_error.load();
    if (st == GL_OK) return GL_OK;
    if (!message[0]) { snprintf(message, sizeof message, "%s: a lane failed", who); return gl_fail(st, message, __FILE__, __LINE__); }
    memcpy(g_gl_last_error, message, sizeof message);      // the failing lane's own text, as it wrote it
    return st;
}
