// Probe behind the small select's profile bracket (select_local in kg_runtime.cpp): does an event pair
// bound by hipExtLaunchKernelGGL report the dispatch's own begin-to-end time? A kernel that spins for a fixed number of
// 100 MHz wall-clock ticks (bounded), timed with a recorded pair, with a pair bound to the one launch, with the start
// bound to a first launch and the stop to a second, and with the pairs reused across the forms (the pool's case).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/event_pair_probe.hip -o tools/event_pair_probe
// Output of one run: profiles/profile_bracket/event_pair_probe.txt
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>

__global__ void spin(unsigned ticks, unsigned* out) {
    const unsigned long long t0 = wall_clock64();
    unsigned n = 0;
    while (wall_clock64() - t0 < ticks && n < (1u << 22)) n++;
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = n;
}

#define CK(x)                                                                  \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            printf("FAIL %s: %s\n", #x, hipGetErrorString(e_));                \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char** argv) {
    // argv[1] = 1: timing-only events (hipEventDisableSystemFence)
    const unsigned evflags = argc > 1 && argv[1][0] == '1' ? hipEventDisableSystemFence : hipEventDefault;
    printf("event flags 0x%x\n", evflags);
    hipStream_t s;
    CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    unsigned* d;
    CK(hipMalloc(&d, 4));
    const int N = 20;
    hipEvent_t a[N], b[N];
    for (int i = 0; i < N; i++) {
        CK(hipEventCreateWithFlags(&a[i], evflags));
        CK(hipEventCreateWithFlags(&b[i], evflags));
    }
    for (unsigned ticks : {1750u, 5000u}) {  // 17.5 us, 50 us
        for (int w = 0; w < 3; w++) spin<<<64, 64, 0, s>>>(ticks, d);
        CK(hipStreamSynchronize(s));
        // 0) no events
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < N; i++) spin<<<64, 64, 0, s>>>(ticks, d);
        CK(hipStreamSynchronize(s));
        auto t2 = std::chrono::steady_clock::now();
        printf("ticks %u no events: wall/step %.4f ms\n", ticks, std::chrono::duration<double, std::milli>(t2 - t0).count() / N);
        // 1) recorded pair
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < N; i++) {
            CK(hipEventRecord(a[i], s));
            spin<<<64, 64, 0, s>>>(ticks, d);
            CK(hipEventRecord(b[i], s));
        }
        auto t1 = std::chrono::steady_clock::now();
        CK(hipStreamSynchronize(s));
        t2 = std::chrono::steady_clock::now();
        float sum = 0, ms;
        for (int i = 0; i < N; i++) {
            CK(hipEventSynchronize(b[i]));
            CK(hipEventElapsedTime(&ms, a[i], b[i]));
            sum += ms;
        }
        printf("ticks %u recorded: bracket %.4f ms, wall/step %.4f ms, submit/step %.4f ms\n", ticks, sum / N,
               std::chrono::duration<double, std::milli>(t2 - t0).count() / N,
               std::chrono::duration<double, std::milli>(t1 - t0).count() / N);
        // 2) ext-bound pair on one kernel (events reused after a record: the pool case)
        t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < N; i++) hipExtLaunchKernelGGL(spin, dim3(64), dim3(64), 0, s, a[i], b[i], 0, ticks, d);
        CK(hipGetLastError());
        t1 = std::chrono::steady_clock::now();
        CK(hipStreamSynchronize(s));
        t2 = std::chrono::steady_clock::now();
        sum = 0;
        float mn = 1e9f, mx = -1e9f;
        for (int i = 0; i < N; i++) {
            CK(hipEventSynchronize(b[i]));
            CK(hipEventElapsedTime(&ms, a[i], b[i]));
            sum += ms;
            mn = ms < mn ? ms : mn;
            mx = ms > mx ? ms : mx;
        }
        printf("ticks %u ext one kernel: bracket %.4f ms (min %.4f max %.4f), wall/step %.4f ms, submit/step %.4f ms\n",
               ticks, sum / N, mn, mx, std::chrono::duration<double, std::milli>(t2 - t0).count() / N,
               std::chrono::duration<double, std::milli>(t1 - t0).count() / N);
        // 3) start bound to a first kernel, stop to a second
        for (int i = 0; i < N; i++) {
            hipExtLaunchKernelGGL(spin, dim3(64), dim3(64), 0, s, a[i], (hipEvent_t) nullptr, 0, ticks, d);
            hipExtLaunchKernelGGL(spin, dim3(64), dim3(64), 0, s, (hipEvent_t) nullptr, b[i], 0, ticks, d);
        }
        CK(hipGetLastError());
        CK(hipStreamSynchronize(s));
        sum = 0;
        for (int i = 0; i < N; i++) {
            CK(hipEventSynchronize(b[i]));
            CK(hipEventElapsedTime(&ms, a[i], b[i]));
            sum += ms;
        }
        printf("ticks %u ext two kernels: bracket %.4f ms\n", ticks, sum / N);
        // 4) a recorded pair again on the same events (pool reuse in the other direction)
        CK(hipEventRecord(a[0], s));
        spin<<<64, 64, 0, s>>>(ticks, d);
        CK(hipEventRecord(b[0], s));
        CK(hipEventSynchronize(b[0]));
        CK(hipEventElapsedTime(&ms, a[0], b[0]));
        printf("ticks %u recorded again: bracket %.4f ms\n", ticks, ms);
    }
    // a fresh, never recorded pair bound by the ext launch
    hipEvent_t c0, c1;
    CK(hipEventCreateWithFlags(&c0, evflags));
    CK(hipEventCreateWithFlags(&c1, evflags));
    hipExtLaunchKernelGGL(spin, dim3(64), dim3(64), 0, s, c0, c1, 0, 1750u, d);
    CK(hipGetLastError());
    CK(hipEventSynchronize(c1));
    float ms;
    CK(hipEventElapsedTime(&ms, c0, c1));
    printf("fresh pair ext: bracket %.4f ms\n", ms);
    CK(hipStreamSynchronize(s));
    printf("probe ok\n");
    return 0;
}
