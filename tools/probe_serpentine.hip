// tools/probe_serpentine.hip -- what does the Infinity Cache keep between two band steps that walk
// their line ranges in opposite directions?.  The band step's walk as in
// tools/membench_layout.hip's k_walk: vector-major rows, a workgroup = half a line of 400 rows (448
// threads, 2 per CU), contiguous line ranges, the next line's loads issued before this line is
// consumed.  A launch reads NV vectors and writes 2; the two it writes are two of the NV the next
// launch reads (as step j's v_j and w are read by step j + 1), ping-pong between two pairs.
// Timed: the second of two back-to-back launches, median of 7 pairs, for
//   directions   ff  both launches walk forward          fr  the second walks every range backwards
//   loads        nt  non-temporal everywhere             pl  plain everywhere
//                ed  plain on the first and last K lines of a range's walk, non-temporal between
//   stores       wt  write-through (sc1) everywhere      pk  plain on the last K lines of the walk
// K: K lines x all ranges x (NV + 2) streams ~ 256 MiB.  If a later step finds the lines the previous
// one touched last, fr is faster than ff by up to 256 MiB / ((NV + 2) x 160 MB) of its time.
// Build: hipcc --offload-arch=gfx950 -O3 -o probe_serpentine tools/probe_serpentine.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHK(x)                                                                               \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess) {                                                              \
            std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));   \
            std::exit(2);                                                                    \
        }                                                                                    \
    } while (0)

__device__ __forceinline__ void st_wt(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct WalkArgs {
    const double *V;    // NV - 2 vectors at k * ld
    const double *r0, *r1;   // the previous launch's outputs: read vectors NV - 2, NV - 1
    double *o0, *o1;
    int64_t n, ld;
    int L, H;
    int rev;     // walk every range backwards
    int lpol;    // 0 nt, 1 plain, 2 plain on the first / last K lines
    int spol;    // 0 write-through, 1 plain on the last K lines
    int K;
};

template <int NV>
__global__ __launch_bounds__(448) void k_walk(WalkArgs a) {
    const int L = a.L, LP = L / a.H, X = (int)(a.n / L);
    const int b = blockIdx.x, R = (int)gridDim.x / a.H, rb = b / a.H, h = b % a.H;
    const int xa = (int)((int64_t)rb * X / R), xb = (int)((int64_t)(rb + 1) * X / R), nl = xb - xa;
    const int t = threadIdx.x;
    if (t >= LP) return;
    auto line = [&](int i) { return a.rev ? xb - 1 - i : xa + i; };
    auto edge = [&](int i) { return i < a.K || i >= nl - a.K; };   // workgroup-uniform
    auto vec = [&](int k) { return k < NV - 2 ? a.V + (int64_t)k * a.ld : (k == NV - 2 ? a.r0 : a.r1); };
    auto load = [&](int i, double *o) {
        const int64_t r = (int64_t)line(i) * L + h * LP + t;
        const bool plain = a.lpol == 1 || (a.lpol == 2 && edge(i));
        if (plain) {
#pragma unroll
            for (int k = 0; k < NV; ++k) o[k] = vec(k)[r];
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) o[k] = __builtin_nontemporal_load(vec(k) + r);
        }
    };
    double nx[NV];
    load(0, nx);
    for (int i = 0; i < nl; ++i) {
        double cu[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) cu[k] = nx[k];
        if (i + 1 < nl) load(i + 1, nx);
        double s = 0.0, c = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            s += cu[k];
            c -= cu[k];
        }
        const int64_t r = (int64_t)line(i) * L + h * LP + t;
        if (a.spol == 1 && i >= nl - a.K) {
            a.o0[r] = s;
            a.o1[r] = c;
        } else {
            st_wt(a.o0 + r, s);
            st_wt(a.o1 + r, c);
        }
    }
}

template <int NV>
static void probe(int64_t n, int ncu) {
    const int L = 800, H = 2;
    const int X = (int)(n / L);
    const int64_t ld = (n + 63) / 64 * 64;
    const int R = std::min(2 * ncu / H, X / 2);
    double *V, *pp[4];
    CHK(hipMalloc(&V, sizeof(double) * (NV - 2) * ld));
    CHK(hipMemset(V, 0, sizeof(double) * (NV - 2) * ld));
    for (auto &p : pp) {
        CHK(hipMalloc(&p, sizeof(double) * ld));
        CHK(hipMemset(p, 0, sizeof(double) * ld));
    }
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0));
    CHK(hipEventCreate(&e1));
    const int K = std::max(1, (int)(268435456.0 / (8.0 * L * R * (NV + 2)) + 0.5));
    const double bytes = 8.0 * n * (NV + 2);
    std::printf("NV %d (+2 written): %.2f GB per launch, %d ranges of ~%d lines, K = %d lines\n", NV, bytes / 1e9, R,
                X / R, K);
    static const char *LN[] = {"nt", "pl", "ed"}, *SN[] = {"wt", "pk"};
    for (int lpol = 0; lpol < 3; ++lpol)
        for (int spol = 0; spol < 2; ++spol) {
            double us[2];
            for (int dir = 0; dir < 2; ++dir) {
                WalkArgs a{V, pp[0], pp[1], pp[2], pp[3], n, ld, L, H, 0, lpol, spol, K};
                WalkArgs c{V, pp[2], pp[3], pp[0], pp[1], n, ld, L, H, dir, lpol, spol, K};
                std::vector<float> ts;
                for (int r = 0; r < 8; ++r) {
                    hipLaunchKernelGGL(k_walk<NV>, dim3(R * H), dim3(448), 0, 0, a);
                    CHK(hipEventRecord(e0));
                    hipLaunchKernelGGL(k_walk<NV>, dim3(R * H), dim3(448), 0, 0, c);
                    CHK(hipEventRecord(e1));
                    CHK(hipEventSynchronize(e1));
                    float ms;
                    CHK(hipEventElapsedTime(&ms, e0, e1));
                    if (r > 0) ts.push_back(ms);   // pair 0: warm-up
                }
                std::sort(ts.begin(), ts.end());
                us[dir] = 1e3 * ts[3];
                std::printf("  NV %2d loads %s stores %s %s  %8.1f us  %7.1f GB/s  (min %.1f max %.1f)\n", NV, LN[lpol],
                            SN[spol], dir ? "fr" : "ff", us[dir], bytes / (1e-6 * us[dir]) / 1e9, 1e3 * ts.front(),
                            1e3 * ts.back());
                std::fflush(stdout);
            }
            std::printf("  NV %2d loads %s stores %s fr/ff = %.3f\n", NV, LN[lpol], SN[spol], us[1] / us[0]);
        }
    CHK(hipEventDestroy(e0));
    CHK(hipEventDestroy(e1));
    CHK(hipFree(V));
    for (auto &p : pp) CHK(hipFree(p));
}

int main(int argc, char **argv) {
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 20000000;
    if (n < 1600 || n > 100000000) return 2;
    int dev = 0, ncu = 0;
    CHK(hipGetDevice(&dev));
    CHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    std::printf("probe_serpentine: n = %lld rows, %d CUs\n", (long long)n, ncu);
    probe<6>(n, ncu);
    probe<12>(n, ncu);
    probe<22>(n, ncu);
    return 0;
}
