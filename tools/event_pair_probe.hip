// Probe behind the small select's profile bracket (select_local in kg_runtime.cpp): does an event pair
// bound by hipExtLaunchKernelGGL report the dispatch's own begin-to-end time? A kernel that spins for a fixed number of
// 100 MHz wall-clock ticks (bounded), timed with a recorded pair, with a pair bound to the one launch, with the start
// bound to a first launch and the stop to a second, and with the pairs reused across the forms (the pool's case).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/event_pair_probe.hip -o tools/event_pair_probe
// Output of one run: profiles/profile_bracket/event_pair_probe.txt
// Fourth leg, "device clock" (DESIGN.md §4 "The bracket is taken inside the launch"): the bracket without any event. Every
// workgroup folds the complement of its entry time into one word (atomic maximum: the word then holds the complement of
// the earliest begin), the workgroup that draws the last ticket takes the word back to zero, reads the clock and adds
// end - begin to a tick counter. Printed beside the plain and the event-bound launch of the same kernel on the same
// grid, with the spread of the workgroups' begin ticks per launch (are the XCDs' clocks one clock?).
// Output of one run: profiles/device_clock/event_pair_probe.txt
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

// The device-clock leg's kernel: spin's loop between the begin fold and k_select_small's hand-off (drain, workgroup
// barrier, returned ticket add). begin / ticket: zero between launches. slots[launch][workgroup]: every workgroup's
// begin; fin[launch]: {earliest begin as the finisher took it, its end}.
__global__ void spin_clock(unsigned ticks, unsigned* out, unsigned long long* begin, unsigned* ticket,
                           unsigned long long* prof, unsigned long long* slots, unsigned long long* fin) {
    __shared__ unsigned last;
    if (begin && threadIdx.x == 0) {  // begin == nullptr: the same kernel and hand-off, nothing timed
        const unsigned long long tb = wall_clock64();
        __hip_atomic_fetch_max(begin, ~tb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (slots) slots[blockIdx.x] = tb;
    }
    const unsigned long long t0 = wall_clock64();
    unsigned n = 0;
    while (wall_clock64() - t0 < ticks && n < (1u << 22)) n++;
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = n;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u;
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!begin) return;
        const unsigned long long b = ~__hip_atomic_exchange(begin, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long te = wall_clock64();
        __hip_atomic_fetch_add(prof, te - b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(prof + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fin) {
            fin[0] = b;
            fin[1] = te;
        }
    }
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
        // 5) device clock: plain launches of spin_clock on more workgroups than compute units; beside it the plain
        // and the event-bound launch on the same grid
        {
            const unsigned WGS = 320;
            int rate_khz = 0;
            CK(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, 0));
            unsigned long long *dw, *dslots, *dfin;  // dw: begin word, {ticks, launches}; ticket on a line of its own
            unsigned* dticket;
            CK(hipMalloc(&dw, 3 * 8));
            CK(hipMalloc(&dticket, 128));
            CK(hipMalloc(&dslots, (size_t)N * WGS * 8));
            CK(hipMalloc(&dfin, (size_t)N * 2 * 8));
            CK(hipMemsetAsync(dw, 0, 3 * 8, s));
            CK(hipMemsetAsync(dticket, 0, 128, s));
            for (int w = 0; w < 3; w++) spin_clock<<<WGS, 64, 0, s>>>(ticks, d, dw, dticket, dw + 1, nullptr, nullptr);
            CK(hipStreamSynchronize(s));
            printf("ticks %u device clock: wall clock rate %d kHz, %u workgroups\n", ticks, rate_khz, WGS);
            for (int rep = 0; rep < 3; rep++) {
                t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; i++) spin<<<WGS, 64, 0, s>>>(ticks, d);
                CK(hipStreamSynchronize(s));
                t2 = std::chrono::steady_clock::now();
                printf("ticks %u rep %d no events, %u workgroups: wall/step %.4f ms\n", ticks, rep, WGS,
                       std::chrono::duration<double, std::milli>(t2 - t0).count() / N);
                // the control: spin_clock with its hand-off, untimed
                t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; i++)
                    spin_clock<<<WGS, 64, 0, s>>>(ticks, d, nullptr, dticket, nullptr, nullptr, nullptr);
                CK(hipStreamSynchronize(s));
                t2 = std::chrono::steady_clock::now();
                printf("ticks %u rep %d no events, same kernel untimed (ticket hand-off, no clock): wall/step %.4f ms\n", ticks,
                       rep, std::chrono::duration<double, std::milli>(t2 - t0).count() / N);
                // device clock, nothing else stored (the form the library runs)
                unsigned long long h0[3], h1[3];
                CK(hipMemcpy(h0, dw, sizeof h0, hipMemcpyDeviceToHost));
                t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; i++) spin_clock<<<WGS, 64, 0, s>>>(ticks, d, dw, dticket, dw + 1, nullptr, nullptr);
                CK(hipGetLastError());
                t1 = std::chrono::steady_clock::now();
                CK(hipStreamSynchronize(s));
                t2 = std::chrono::steady_clock::now();
                CK(hipMemcpy(h1, dw, sizeof h1, hipMemcpyDeviceToHost));
                const double dticks = (double)(h1[1] - h0[1]) / N;
                printf("ticks %u rep %d device clock: bracket %.1f ticks = %.4f ms (launches %llu, begin word after %llu), "
                       "wall/step %.4f ms, submit/step %.4f ms\n",
                       ticks, rep, dticks, rate_khz ? dticks / rate_khz : 0.0, h1[2] - h0[2], h1[0],
                       std::chrono::duration<double, std::milli>(t2 - t0).count() / N,
                       std::chrono::duration<double, std::milli>(t1 - t0).count() / N);
                // the bound pair on the same kernel
                t0 = std::chrono::steady_clock::now();
                for (int i = 0; i < N; i++)
                    hipExtLaunchKernelGGL(spin_clock, dim3(WGS), dim3(64), 0, s, a[i], b[i], 0, ticks, d, dw, dticket, dw + 1,
                                          (unsigned long long*)nullptr, (unsigned long long*)nullptr);
                CK(hipGetLastError());
                CK(hipStreamSynchronize(s));
                t2 = std::chrono::steady_clock::now();
                unsigned long long h2[3];
                CK(hipMemcpy(h2, dw, sizeof h2, hipMemcpyDeviceToHost));
                sum = 0;
                for (int i = 0; i < N; i++) {
                    CK(hipEventElapsedTime(&ms, a[i], b[i]));
                    sum += ms;
                }
                const double eticks = (double)(h2[1] - h1[1]) / N;
                printf("ticks %u rep %d ext one kernel, %u workgroups: bracket %.4f ms (device clock of the same launches "
                       "%.4f ms: shorter by %.4f ms), wall/step %.4f ms\n",
                       ticks, rep, WGS, sum / N, rate_khz ? eticks / rate_khz : 0.0,
                       sum / N - (rate_khz ? eticks / rate_khz : 0.0),
                       std::chrono::duration<double, std::milli>(t2 - t0).count() / N);
            }
            // per launch: every workgroup's begin, and the finisher's pair
            for (int i = 0; i < N; i++)
                spin_clock<<<WGS, 64, 0, s>>>(ticks, d, dw, dticket, dw + 1, dslots + (size_t)i * WGS, dfin + (size_t)i * 2);
            CK(hipGetLastError());
            CK(hipStreamSynchronize(s));
            static unsigned long long hs[20 * 320], hf[20 * 2];
            CK(hipMemcpy(hs, dslots, (size_t)N * WGS * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hf, dfin, (size_t)N * 2 * 8, hipMemcpyDeviceToHost));
            bool all_ok = true;
            unsigned long long worst = 0;
            for (int i = 0; i < N; i++) {
                unsigned long long mn = ~0ull, mx = 0, xmn[8], xmx[8];
                for (int x = 0; x < 8; x++) xmn[x] = ~0ull, xmx[x] = 0;
                for (unsigned w = 0; w < WGS; w++) {
                    const unsigned long long v = hs[(size_t)i * WGS + w];
                    mn = v < mn ? v : mn;
                    mx = v > mx ? v : mx;
                    xmn[w & 7] = v < xmn[w & 7] ? v : xmn[w & 7];  // workgroups go to the XCDs round robin
                    xmx[w & 7] = v > xmx[w & 7] ? v : xmx[w & 7];
                }
                const bool ok = hf[i * 2] == mn && hf[i * 2 + 1] >= mx;
                all_ok = all_ok && ok;
                worst = mx - mn > worst ? mx - mn : worst;
                if (i < 4 || !ok) {
                    printf("ticks %u launch %d: begin spread %llu ticks, finisher begin %s earliest, end - last begin %lld, "
                           "bracket %llu; first begin per XCD (minus earliest):",
                           ticks, i, mx - mn, hf[i * 2] == mn ? "==" : "!=", (long long)(hf[i * 2 + 1] - mx),
                           hf[i * 2 + 1] - hf[i * 2]);
                    for (int x = 0; x < 8; x++) printf(" %llu", xmn[x] - mn);
                    printf("\n");
                }
            }
            printf("ticks %u device clock: %d launches, widest begin spread %llu ticks, every end >= every begin and finisher "
                   "begin == earliest: %s\n", ticks, N, worst, all_ok ? "yes" : "NO");
            CK(hipFree(dw));
            CK(hipFree(dticket));
            CK(hipFree(dslots));
            CK(hipFree(dfin));
        }
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
