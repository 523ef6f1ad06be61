// Which kinds of HIP stream get a hardware queue of their own?  The runtime multiplexes a process's streams onto at most
// GPU_MAX_HW_QUEUES hardware queues per priority class; a CU-masked stream is believed to bypass that pool.  This program makes
// 8 streams of each kind, launches a few one-block kernels of a fixed duration on every stream, and prints per kind
//   - the flags of the first stream (hipExtStreamCreateWithCUMask takes none: is its stream a blocking one?),
//   - the wall time of 8 streams x 4 kernels against the time of 4 kernels on one stream (n distinct queues give 8 / n times it).
// Each kind launches its own instantiation k_probe<KIND>, so that tools/queue_probe.py can count the distinct queue ids per kind
// in the kernel trace of a rocprofv3 run of this program.  Stand-alone:
//   hipcc --offload-arch=gfx950 -O2 -o tools/queue_probe tools/queue_probe.hip
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// one wave that lasts `ticks` of the 100 MHz wall clock; touches no memory but its one result word
template <int KIND>
__global__ void k_probe(uint64_t ticks, uint64_t* out) {
    const uint64_t t0 = wall_clock64();
    uint64_t t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (threadIdx.x == 0 && out) out[blockIdx.x] = t - t0;
}

static const int STREAMS = 8, LAUNCHES = 4;
static const uint64_t TICKS = 20000;      // 200 us

template <int KIND>
static int run_kind(const char* what, std::vector<hipStream_t>& ss) {
    unsigned flags = ~0u; int prio = 99;
    CHECK(hipStreamGetFlags(ss[0], &flags));
    CHECK(hipStreamGetPriority(ss[0], &prio));
    // warm every stream (first use may be what binds it to a queue)
    for (hipStream_t s : ss) k_probe<KIND><<<1, 64, 0, s>>>(100, nullptr);
    for (hipStream_t s : ss) CHECK(hipStreamSynchronize(s));
    auto t0 = std::chrono::steady_clock::now();
    for (int l = 0; l < LAUNCHES; l++) k_probe<KIND><<<1, 64, 0, ss[0]>>>(TICKS, nullptr);
    CHECK(hipStreamSynchronize(ss[0]));
    const double one = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    t0 = std::chrono::steady_clock::now();
    for (int l = 0; l < LAUNCHES; l++) for (hipStream_t s : ss) k_probe<KIND><<<1, 64, 0, s>>>(TICKS, nullptr);
    for (hipStream_t s : ss) CHECK(hipStreamSynchronize(s));
    const double all = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("kind %d  %-44s flags 0x%x (%s)  priority %d  one stream %7.0f us  %d streams %7.0f us  ratio %.2f\n", KIND, what, flags,
           (flags & hipStreamNonBlocking) ? "non-blocking" : "BLOCKING", prio, one, STREAMS, all, all / one);
    CHECK(hipGetLastError());
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    int least = 0, greatest = 0;
    CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const char* q = getenv("GPU_MAX_HW_QUEUES");
    printf("device %s  CUs %d  GPU_MAX_HW_QUEUES %s  stream priorities %d (least) .. %d (greatest)\n", prop.name, prop.multiProcessorCount,
           q ? q : "(unset)", least, greatest);
    printf("%d streams per kind, %d launches of %llu us on each\n", STREAMS, LAUNCHES, (unsigned long long)(TICKS / 100));

    std::vector<hipStream_t> plain(STREAMS), masked(STREAMS), lo(STREAMS), mid(STREAMS), hi(STREAMS);
    std::vector<uint32_t> mask((prop.multiProcessorCount + 31) / 32, 0);
    for (int cu = 0; cu < prop.multiProcessorCount; cu++) mask[cu / 32] |= 1u << (cu % 32);
    for (int i = 0; i < STREAMS; i++) {
        CHECK(hipStreamCreateWithFlags(&plain[i], hipStreamNonBlocking));
        CHECK(hipExtStreamCreateWithCUMask(&masked[i], (uint32_t)mask.size(), mask.data()));
        CHECK(hipStreamCreateWithPriority(&lo[i], hipStreamNonBlocking, least));
        CHECK(hipStreamCreateWithPriority(&mid[i], hipStreamNonBlocking, (least + greatest) / 2));
        CHECK(hipStreamCreateWithPriority(&hi[i], hipStreamNonBlocking, greatest));
    }
    if (run_kind<0>("hipStreamCreateWithFlags(NonBlocking)", plain)) return 1;
    if (run_kind<1>("hipExtStreamCreateWithCUMask(all CUs)", masked)) return 1;
    if (run_kind<2>("hipStreamCreateWithPriority(least)", lo)) return 1;
    if (run_kind<3>("hipStreamCreateWithPriority(middle)", mid)) return 1;
    if (run_kind<4>("hipStreamCreateWithPriority(greatest)", hi)) return 1;
    // all three priority classes at once: 24 streams
    {
        std::vector<hipStream_t> all3;
        for (int i = 0; i < STREAMS; i++) { all3.push_back(lo[i]); all3.push_back(mid[i]); all3.push_back(hi[i]); }
        auto t0 = std::chrono::steady_clock::now();
        for (int l = 0; l < LAUNCHES; l++) for (hipStream_t s : all3) k_probe<5><<<1, 64, 0, s>>>(TICKS, nullptr);
        for (hipStream_t s : all3) CHECK(hipStreamSynchronize(s));
        const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("kind 5  the 24 streams of kinds 2, 3 and 4 together: %7.0f us (one queue each would be %d us, one queue for all %d us)\n", t,
               (int)(LAUNCHES * TICKS / 100), (int)(24 * LAUNCHES * TICKS / 100));
    }
    // plain and masked together: do the masked streams leave the pool's queues to the plain ones?
    {
        std::vector<hipStream_t> both;
        for (int i = 0; i < STREAMS; i++) { both.push_back(plain[i]); both.push_back(masked[i]); }
        auto t0 = std::chrono::steady_clock::now();
        for (int l = 0; l < LAUNCHES; l++) for (hipStream_t s : both) k_probe<6><<<1, 64, 0, s>>>(TICKS, nullptr);
        for (hipStream_t s : both) CHECK(hipStreamSynchronize(s));
        const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("kind 6  the 16 streams of kinds 0 and 1 together:    %7.0f us\n", t);
    }
    for (int i = 0; i < STREAMS; i++) {
        CHECK(hipStreamDestroy(plain[i])); CHECK(hipStreamDestroy(masked[i]));
        CHECK(hipStreamDestroy(lo[i])); CHECK(hipStreamDestroy(mid[i])); CHECK(hipStreamDestroy(hi[i]));
    }
    return 0;
}
