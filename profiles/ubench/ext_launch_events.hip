// What the start and stop events of hipExtLaunchKernelGGL give on this runtime: elapsed time within and across
// kernels, order through a stop event, a wait after the stream is gone, and what markers cost between two dependent
// kernels (tiny ones, then 100 us ones).  Results: profiles/step_markers/ext_launch_events.txt
//   hipcc --offload-arch=gfx950 -O2 -o ext_launch_events ext_launch_events.hip
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <chrono>
#include <cstdio>
#include <vector>

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            printf("FAIL %s -> %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);      \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

__global__ void k_spin(long long ticks, int *flag, int value) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {
    }
    if (flag && threadIdx.x == 0 && blockIdx.x == 0) *flag = value;
}
__global__ void k_read(const int *flag, int *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = *flag;
}
__global__ void k_tiny(int *p) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *p += 1;
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main() {
    int *flag, *out;
    CK(hipMalloc(&flag, 4));
    CK(hipMalloc(&out, 4));
    CK(hipMemset(flag, 0, 4));
    CK(hipMemset(out, 0, 4));
    hipStream_t s1, s2;
    CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    CK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    const long long us100 = 100 * 100;  // wall_clock64 runs at 100 MHz

    // 1. elapsed time within and across kernels
    {
        hipEvent_t r0, r1, r2, a0, a1, b0, b1;
        for (hipEvent_t *e : {&r0, &r1, &r2, &a0, &a1, &b0, &b1}) CK(hipEventCreate(e));
        k_spin<<<1, 64, 0, s1>>>(us100, nullptr, 0);
        CK(hipStreamSynchronize(s1));
        CK(hipEventRecord(r0, s1));
        hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, a0, a1, 0, 2 * us100, (int *)nullptr, 0);
        CK(hipGetLastError());
        CK(hipEventRecord(r1, s1));
        hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, b0, b1, 0, us100, (int *)nullptr, 0);
        CK(hipGetLastError());
        CK(hipEventRecord(r2, s1));
        printf("query before sync: a1=%d b1=%d\n", (int)hipEventQuery(a1), (int)hipEventQuery(b1));
        CK(hipStreamSynchronize(s1));
        printf("query after sync: a0=%d a1=%d b0=%d b1=%d\n", (int)hipEventQuery(a0), (int)hipEventQuery(a1), (int)hipEventQuery(b0), (int)hipEventQuery(b1));
        float t;
        hipError_t e;
        e = hipEventElapsedTime(&t, r0, r1); printf("record r0->r1 (A ~0.2): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, r1, r2); printf("record r1->r2 (B ~0.1): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, a0, a1); printf("ext a0->a1 (A): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, b0, b1); printf("ext b0->b1 (B): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, a0, b1); printf("ext a0->b1 (A+B ~0.3): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, a1, b0); printf("ext a1->b0 (gap): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, a1, b1); printf("ext a1->b1 (B+gap): %d %.4f\n", (int)e, t);
        e = hipEventElapsedTime(&t, a0, b0); printf("ext a0->b0 (A+gap): %d %.4f\n", (int)e, t);
        (void)hipGetLastError();
        // one start event bound to kernel A, one stop event bound to kernel B (the issue's preferred form)
        hipEvent_t c0, c1;
        CK(hipEventCreate(&c0));
        CK(hipEventCreate(&c1));
        hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, c0, nullptr, 0, 2 * us100, (int *)nullptr, 0);
        printf("start-only launch: %d\n", (int)hipGetLastError());
        hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, nullptr, c1, 0, us100, (int *)nullptr, 0);
        printf("stop-only launch: %d\n", (int)hipGetLastError());
        CK(hipStreamSynchronize(s1));
        e = hipEventElapsedTime(&t, c0, c1); printf("ext c0(start of A)->c1(stop of B) (~0.3): %d %.4f\n", (int)e, t);
        (void)hipGetLastError();
    }

    // 2. ordering through a stop event without timing, re-bound to two kernels; 3. after the stream is destroyed
    {
        hipEvent_t ev;
        CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        int bad = 0;
        for (int rep = 0; rep < 20; ++rep) {
            CK(hipMemsetAsync(flag, 0, 4, s1));
            CK(hipStreamSynchronize(s1));
            hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, nullptr, ev, 0, 3 * us100, flag, 1);
            CK(hipGetLastError());
            hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, nullptr, ev, 0, 3 * us100, flag, 2);
            CK(hipGetLastError());
            CK(hipStreamWaitEvent(s2, ev, 0));
            k_read<<<1, 64, 0, s2>>>(flag, out);
            CK(hipGetLastError());
            CK(hipStreamSynchronize(s2));
            int h = -1;
            CK(hipMemcpy(&h, out, 4, hipMemcpyDeviceToHost));
            if (h != 2) ++bad;
            CK(hipStreamSynchronize(s1));
        }
        printf("ordering through a re-bound stop event (no timing): %d of 20 wrong\n", bad);
        hipStream_t s3;
        CK(hipStreamCreateWithFlags(&s3, hipStreamNonBlocking));
        hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s3, nullptr, ev, 0, us100, flag, 7);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(s3));
        CK(hipStreamDestroy(s3));
        hipError_t e = hipStreamWaitEvent(s2, ev, 0);
        printf("wait on the event after its stream was destroyed: %d\n", (int)e);
        k_read<<<1, 64, 0, s2>>>(flag, out);
        CK(hipStreamSynchronize(s2));
        int h = -1;
        CK(hipMemcpy(&h, out, 4, hipMemcpyDeviceToHost));
        printf("  read %d (want 7)\n", h);
    }

    // 4. what markers cost between two dependent tiny kernels
    {
        const int steps = 2000;
        std::vector<hipEvent_t> pool(6);
        for (auto &e : pool) CK(hipEventCreate(&e));
        hipEvent_t tail;
        CK(hipEventCreateWithFlags(&tail, hipEventDisableTiming));
        for (int round = 0; round < 3; ++round)
            for (int mode = 0; mode < 5; ++mode) {
                CK(hipStreamSynchronize(s1));
                const double t0 = now_ms();
                for (int i = 0; i < steps; ++i) {
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[0], s1));
                    if (mode == 3 || mode == 4) hipExtLaunchKernelGGL(k_tiny, dim3(1), dim3(64), 0, s1, pool[0], pool[1], 0, flag);
                    else k_tiny<<<1, 64, 0, s1>>>(flag);
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[1], s1));
                    if (mode == 3) hipExtLaunchKernelGGL(k_tiny, dim3(1), dim3(64), 0, s1, pool[2], pool[3], 0, flag);
                    else if (mode == 4) hipExtLaunchKernelGGL(k_tiny, dim3(1), dim3(64), 0, s1, pool[2], tail, 0, flag);
                    else k_tiny<<<1, 64, 0, s1>>>(flag);
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[2], s1));
                    if (mode == 2) CK(hipEventRecord(tail, s1));
                }
                CK(hipStreamSynchronize(s1));
                const double dt = now_ms() - t0;
                static const char *names[] = {"plain", "3 records", "3 records + tail record", "ext pairs", "ext pairs, tail as stop"};
                printf("round %d  %-26s %.3f us per step of two kernels\n", round, names[mode], dt * 1e3 / steps);
            }
    }
    // 5. the same with two 100 us kernels: the excess over 200 us is what the stream carries besides them
    {
        const int steps = 300;
        std::vector<hipEvent_t> pool(6);
        for (auto &e : pool) CK(hipEventCreate(&e));
        hipEvent_t tail;
        CK(hipEventCreateWithFlags(&tail, hipEventDisableTiming));
        for (int round = 0; round < 3; ++round)
            for (int mode = 0; mode < 7; ++mode) {
                CK(hipStreamSynchronize(s1));
                const double t0 = now_ms();
                for (int i = 0; i < steps; ++i) {
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[0], s1));
                    if (mode == 3 || mode == 4) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, pool[0], pool[1], 0, us100, flag, 1);
                    else k_spin<<<1, 64, 0, s1>>>(us100, flag, 1);
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[1], s1));
                    if (mode == 3) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, pool[2], pool[3], 0, us100, flag, 1);
                    else if (mode == 6) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, nullptr, tail, 0, us100, flag, 1);
                    else if (mode == 4) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, pool[2], tail, 0, us100, flag, 1);
                    else k_spin<<<1, 64, 0, s1>>>(us100, flag, 1);
                    if (mode == 1 || mode == 2) CK(hipEventRecord(pool[2], s1));
                    if (mode == 2 || mode == 5) CK(hipEventRecord(tail, s1));
                }
                CK(hipStreamSynchronize(s1));
                const double dt = now_ms() - t0;
                static const char *names[] = {"plain", "3 records", "3 records + tail record", "ext pairs", "ext pairs, tail as stop", "plain + tail record", "plain, tail as stop of 2nd"};
                printf("round %d  %-26s %.3f us per step of two 100 us kernels\n", round, names[mode], dt * 1e3 / steps);
            }
    }
    printf("DONE\n");
    return 0;
}
