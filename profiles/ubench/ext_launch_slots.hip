// Which event slot of hipExtLaunchKernelGGL costs stream time: two dependent 100 us kernels per step with start-only,
// stop-only and paired events of each kind.  Results: profiles/step_markers/ext_launch_slots.txt (a stop event is
// free, a start event costs what a recorded one does).
//   hipcc --offload-arch=gfx950 -O2 -o ext_launch_slots ext_launch_slots.hip
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <chrono>
#include <cstdio>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("FAIL %s -> %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); return 1; } } while (0)
__global__ void k_spin(long long ticks, int *flag, int value) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) {}
    if (flag && threadIdx.x == 0 && blockIdx.x == 0) *flag = value;
}
static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int main() {
    int *flag;
    CK(hipMalloc(&flag, 4));
    hipStream_t s1;
    CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    const long long us100 = 100 * 100;
    hipEvent_t t[4], nt[4], nf[4];
    for (auto &e : t) CK(hipEventCreate(&e));
    for (auto &e : nt) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : nf) CK(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
    static const char *names[] = {"plain", "stop-only timing x2", "start-only timing x2", "pairs no-timing x2", "k1 pair + k2 stop-only", "pairs no-system-fence x2",
                                  "pairs timing x2", "k1 start-only + k2 stop-only", "stop-only no-system-fence x2"};
    struct M { hipEvent_t a0, a1, b0, b1; };
    M modes[] = {{0, 0, 0, 0}, {0, t[1], 0, t[3]}, {t[0], 0, t[2], 0}, {nt[0], nt[1], nt[2], nt[3]}, {t[0], t[1], 0, t[3]}, {nf[0], nf[1], nf[2], nf[3]},
                 {t[0], t[1], t[2], t[3]}, {t[0], 0, 0, t[3]}, {0, nf[1], 0, nf[3]}};
    const int steps = 300;
    for (int round = 0; round < 3; ++round)
        for (int mode = 0; mode < 9; ++mode) {
            const M &m = modes[mode];
            CK(hipStreamSynchronize(s1));
            const double t0 = now_ms();
            for (int i = 0; i < steps; ++i) {
                if (m.a0 || m.a1) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, m.a0, m.a1, 0, us100, flag, 1);
                else k_spin<<<1, 64, 0, s1>>>(us100, flag, 1);
                if (m.b0 || m.b1) hipExtLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s1, m.b0, m.b1, 0, us100, flag, 1);
                else k_spin<<<1, 64, 0, s1>>>(us100, flag, 1);
            }
            CK(hipStreamSynchronize(s1));
            const double dt = now_ms() - t0;
            float el = -1.f;
            if (m.a0 && m.b1 && mode != 3) (void)hipEventElapsedTime(&el, m.a0, m.b1);
            (void)hipGetLastError();
            printf("round %d  %-30s %.3f us per step   (elapsed first.start->last.stop %.4f ms)\n", round, names[mode], dt * 1e3 / steps, el);
        }
    printf("DONE\n");
    return 0;
}
