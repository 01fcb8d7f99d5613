// vtk_line2.hip — the line product's second sweep.
//
// M = M1 D^-1 M2 with M1, M2 two line-Jacobi matrices of A (two (stride, seg) pairs) and D A's
// diagonal; M^-1 r = M2^-1 (D (M1^-1 r)).  The first sweep is k_line_apply on direction 1
// (vtk_kernels.hip, unchanged); this file holds the second: the same Thomas sweeps on direction
// 2's factors with the forward right-hand side formed as D[k] t[k] per row, so u = D t is never
// stored.  Built with -ffp-contract=off: the product D[k] t[k] is rounded before the subtraction,
// and the result is bit-identical to orc_line_apply(lf2, D * orc_line_apply(lf1, r)).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vtk_internal.hpp"
#include "vtk_device.hpp"

namespace vtk {

// D[r] = sum of row r's stored entries with col == row (local numbering), in stored order from
// 0.0 in double, float32 values widened first: the b of k_line_setup
template <typename VT>
__global__ __launch_bounds__(NT) void k_line2_diag(const int32_t *__restrict__ indptr,
                                                   const int32_t *__restrict__ indices,
                                                   const VT *__restrict__ data, int64_t n, double *__restrict__ D) {
    for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (int64_t)gridDim.x * NT) {
        double b = 0.0;
        for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k)
            if ((int64_t)indices[k] == r) b += (double)data[k];
        D[r] = b;
    }
}

// z = M_L^-1 (D t): one lane per (segment, j) as in k_line_apply; forward d = D t - l d_prev,
// backward z = m d - g z_next.  LMAX > 0: the lane's rows in registers, every load of the sweep
// issued before its recurrence (addresses clamped to row 0 off the block, results discarded).
// COMPACT: l = a m_prev and g = c m from the line's constant couplings (L.ac): t, D and m are
// read, 24 B/row, and z written.  LMAX == 0 (segments longer than 32): d goes through z.  t and
// z may alias (each row is read before it is written, by its lane).
// DCD: the DCGS2 step's dots behind the sweep, in k_line_apply<.., true>'s partial layout.
// ACC: the backward sweep stores dc.acc[k] + z[k] (k_line_apply's ACC; z must not alias acc).
template <int LMAX, bool COMPACT, bool DCD = false, bool ACC = false>
__global__ __launch_bounds__(NT) void k_line2_apply(LineOp L, const double *__restrict__ D, const double *t_in,
                                                    double *z, const double *__restrict__ v0, double *part0,
                                                    double *part1, const int *stop_col, int col,
                                                    typename LineDcOf<ACC>::type dc = {}) {
    __shared__ double red[NT / 64];
    constexpr int NQW = 2 * DC_MAXJ + 3;
    __shared__ double stage[DCD ? (NT / 64) * NQW : 1];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nseg * L.jb, S = L.stride, r0 = L.row0, r_end = L.row0 + L.n;
    const double *l = L.f, *m = L.f + L.n, *g = L.f + 2 * L.n;
    double acc0 = 0.0, acc1 = 0.0;
    [[maybe_unused]] double dsl = 0.0, dzl = 0.0, daa = 0.0, dab = 0.0, dag = 0.0;   // DCD
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LineLane q = line_lane(L, t, lane);
        const int64_t len = q.i_end - q.i_beg;
        if constexpr (LMAX > 0) {
            // row offsets k_u = k0 + u*S fit 32 bits (n_local < 2^31)
            const int64_t k0l = q.i_beg * S + q.j - r0;
            const int nn = (int)L.n;
            double aj = 0.0, cj = 0.0;
            if constexpr (COMPACT) {
                if (q.jv) {
                    aj = L.ac[q.j - L.j0];
                    cj = L.ac[L.jn + q.j - L.j0];
                }
            }
            double e[LMAX], gg[LMAX];
            double dp = 0.0, mp = 0.0;
            bool pok = false;
            unsigned okm = 0;
#pragma unroll
            for (int u = 0; u < LMAX; ++u) {
                const int64_t kl = k0l + (int64_t)u * S;
                const bool ok = q.jv && u < len && kl >= 0 && kl < nn;
                const int k = ok ? (int)kl : 0;
                const double mv = ld_nt<8>(m + k);
                double lv, gv;
                if constexpr (COMPACT) {
                    const bool hl = ok && pok;
                    const bool hr = ok && u + 1 < len && kl + S < nn;
                    lv = hl ? aj * mp : 0.0;
                    gv = (hr ? cj : 0.0) * mv;
                } else {
                    lv = l[k];
                    gv = g[k];
                }
                const double uv = ld_nt<8>(D + k) * ld_nt<8>(t_in + k);   // u = D t, rounded here
                const double dv = uv - lv * dp;
                e[u] = mv * dv;
                gg[u] = gv;
                if (ok) {
                    dp = dv;
                    mp = mv;
                }
                pok = ok;
                okm |= (unsigned)ok << u;
            }
            double zn = 0.0;
#pragma unroll
            for (int u = LMAX - 1; u >= 0; --u) {
                const double zv = e[u] - gg[u] * zn;
                if constexpr (ACC) {
                    double zo = 0.0;   // the row's output: acc + z
                    if ((okm >> u) & 1u) {
                        const int k = (int)(k0l + (int64_t)u * S);
                        zo = dc.acc[k] + zv;
                        st_nt<4>(z + k, zo);
                        zn = zv;
                        if constexpr (!DCD) {
                            acc0 += zo * zo;
                            if (v0) acc1 += v0[k] * zo;
                        }
                    }
                    if constexpr (DCD) e[u] = zo;
                    continue;
                }
                if ((okm >> u) & 1u) {
                    const int k = (int)(k0l + (int64_t)u * S);
                    st_nt<4>(z + k, zv);
                    zn = zv;
                    if constexpr (!DCD) {
                        acc0 += zv * zv;
                        if (v0) acc1 += v0[k] * zv;
                    }
                }
                if constexpr (DCD) e[u] = ((okm >> u) & 1u) ? zv : 0.0;   // w, kept for the dots
            }
            if constexpr (DCD) {
                // p on the lane's rows (gg is free after the sweep), then the basis vector by
                // vector; lane k keeps the running sums of vector k (k_line_apply's DCD)
#pragma unroll
                for (int u = 0; u < LMAX; ++u) {
                    const int k = (int)(k0l + (int64_t)u * S);
                    gg[u] = ((okm >> u) & 1u) ? ld_nt<4>(dc.p + k) : 0.0;
                }
#pragma unroll
                for (int u = 0; u < LMAX; ++u) {
                    daa += gg[u] * gg[u];
                    dab += gg[u] * e[u];
                    dag += e[u] * e[u];
                }
                for (int kk = 0; kk < dc.j; ++kk) {
                    const double *vk = dc.V + (size_t)kk * dc.ld;
                    double sl = 0.0, zl = 0.0;
#pragma unroll
                    for (int u = 0; u < LMAX; ++u) {
                        const int k = (int)(k0l + (int64_t)u * S);
                        const double v = ((okm >> u) & 1u) ? __builtin_nontemporal_load(vk + k) : 0.0;
                        sl += v * gg[u];
                        zl += v * e[u];
                    }
                    const double ts = wave_allsum(sl), tz = wave_allsum(zl);
                    if (lane == kk) {
                        dsl += ts;
                        dzl += tz;
                    }
                }
            }
        } else {
            double dp = 0.0;
            for (int64_t u = 0; u < len; ++u) {
                const int64_t R = (q.i_beg + u) * S + q.j;
                if (!q.jv || R < r0 || R >= r_end) continue;
                const int64_t k = R - r0;
                const double uv = D[k] * t_in[k];
                const double dv = uv - l[k] * dp;
                z[k] = dv;
                dp = dv;
            }
            double zn = 0.0;
            for (int64_t u = len - 1; u >= 0; --u) {
                const int64_t R = (q.i_beg + u) * S + q.j;
                if (!q.jv || R < r0 || R >= r_end) continue;
                const int64_t k = R - r0;
                const double zv = m[k] * z[k] - g[k] * zn;
                if constexpr (ACC) {
                    const double zo = dc.acc[k] + zv;
                    z[k] = zo;
                    zn = zv;
                    acc0 += zo * zo;
                    if (v0) acc1 += v0[k] * zo;
                    continue;
                }
                z[k] = zv;
                zn = zv;
                acc0 += zv * zv;
                if (v0) acc1 += v0[k] * zv;
            }
        }
    }
    if constexpr (DCD) {
        // per-workgroup partials: the 4 waves' records summed in wave order
        double *rec = stage + wv * NQW;
        if (lane < dc.j) {
            rec[lane] = dsl;
            rec[DC_MAXJ + lane] = dzl;
        }
        const double t0 = wave_sum(daa), t1 = wave_sum(dab), t2 = wave_sum(dag);
        if (lane == 0) {
            rec[2 * DC_MAXJ] = t0;
            rec[2 * DC_MAXJ + 1] = t1;
            rec[2 * DC_MAXJ + 2] = t2;
        }
        __syncthreads();
        for (int qq = threadIdx.x; qq < DC_NQ; qq += NT) {
            const bool used = qq < dc.j || (qq >= DC_MAXJ && qq < DC_MAXJ + dc.j) || qq >= 2 * DC_MAXJ;
            if (used) {
                double tt = 0.0;
#pragma unroll
                for (int w2 = 0; w2 < NT / 64; ++w2) tt += stage[w2 * NQW + qq];
                dc.part[(size_t)qq * GMAX + blockIdx.x] = tt;
            }
        }
        return;
    }
    if (part0) {
        const double t0 = block_sum(acc0, red);
        if (threadIdx.x == 0) part0[blockIdx.x] = t0;
    }
    if (part1 && v0) {
        const double t1 = block_sum(acc1, red);
        if (threadIdx.x == 0) part1[blockIdx.x] = t1;
    }
}

hipError_t launch_line2_diag(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                             double *D, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 g((unsigned)std::min<int64_t>((n + NT - 1) / NT, 8 * GMAX));
    if (fp32) hipLaunchKernelGGL(k_line2_diag<float>, g, dim3(NT), 0, s, indptr, indices, (const float *)data, n, D);
    else hipLaunchKernelGGL(k_line2_diag<double>, g, dim3(NT), 0, s, indptr, indices, (const double *)data, n, D);
    return hipGetLastError();
}

hipError_t launch_line2_dc(const LineOp &L, const double *D, const double *t, double *w, const double *V, int64_t ld,
                           int j, const double *p, double *part, int grid, const int *stop_col, int col,
                           hipStream_t s, const double *zadd) {
    if (j > DC_MAXJ || grid > GMAX || L.seg > 32 || L.seg <= 0 || !D || zadd == w) return hipErrorInvalidValue;
    const dim3 g(grid), b(NT);
    const LineDc dc{V, ld, j, p, part};
    if (zadd) {   // w = zadd + M_L^-1 (D t) and the dots of that w
        const LineDcAcc da{dc, zadd};
#define VTK_LINE2_DCA_LAUNCH(LM)                                                                             \
    do {                                                                                                     \
        if (L.compact) hipLaunchKernelGGL((k_line2_apply<LM, true, true, true>), g, b, 0, s, L, D, t, w, nullptr, nullptr, nullptr, stop_col, col, da); \
        else hipLaunchKernelGGL((k_line2_apply<LM, false, true, true>), g, b, 0, s, L, D, t, w, nullptr, nullptr, nullptr, stop_col, col, da);        \
    } while (0)
        if (L.seg <= 8) VTK_LINE2_DCA_LAUNCH(8);
        else if (L.seg <= 16) VTK_LINE2_DCA_LAUNCH(16);
        else if (L.seg <= 25) VTK_LINE2_DCA_LAUNCH(25);
        else VTK_LINE2_DCA_LAUNCH(32);
#undef VTK_LINE2_DCA_LAUNCH
        return hipGetLastError();
    }
#define VTK_LINE2_DC_LAUNCH(LM)                                                                              \
    do {                                                                                                     \
        if (L.compact) hipLaunchKernelGGL((k_line2_apply<LM, true, true>), g, b, 0, s, L, D, t, w, nullptr, nullptr, nullptr, stop_col, col, dc); \
        else hipLaunchKernelGGL((k_line2_apply<LM, false, true>), g, b, 0, s, L, D, t, w, nullptr, nullptr, nullptr, stop_col, col, dc);        \
    } while (0)
    if (L.seg <= 8) VTK_LINE2_DC_LAUNCH(8);
    else if (L.seg <= 16) VTK_LINE2_DC_LAUNCH(16);
    else if (L.seg <= 25) VTK_LINE2_DC_LAUNCH(25);
    else VTK_LINE2_DC_LAUNCH(32);
#undef VTK_LINE2_DC_LAUNCH
    return hipGetLastError();
}

hipError_t launch_line2_apply(const LineOp &L, const double *D, const double *t, double *z, const double *v0,
                              double *part0, double *part1, int grid, const int *stop_col, int col, hipStream_t s,
                              const double *zadd) {
    if (L.n == 0 && part0 == nullptr) return hipSuccess;
    if (!D || grid < 1) return hipErrorInvalidValue;
    const dim3 g(grid), b(NT);
    if (zadd) {   // z = zadd + M_L^-1 (D t)
        if (zadd == z) return hipErrorInvalidValue;
        const LineDcAcc da{LineDc{}, zadd};
#define VTK_LINE2_ACC_LAUNCH(LM)                                                                             \
    do {                                                                                                     \
        if (L.compact) hipLaunchKernelGGL((k_line2_apply<LM, true, false, true>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col, da); \
        else hipLaunchKernelGGL((k_line2_apply<LM, false, false, true>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col, da);        \
    } while (0)
        if (L.seg <= 8) VTK_LINE2_ACC_LAUNCH(8);
        else if (L.seg <= 16) VTK_LINE2_ACC_LAUNCH(16);
        else if (L.seg <= 25) VTK_LINE2_ACC_LAUNCH(25);
        else if (L.seg <= 32) VTK_LINE2_ACC_LAUNCH(32);
        else hipLaunchKernelGGL((k_line2_apply<0, false, false, true>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col, da);
#undef VTK_LINE2_ACC_LAUNCH
        return hipGetLastError();
    }
#define VTK_LINE2_LAUNCH(LM)                                                                                 \
    do {                                                                                                     \
        if (L.compact) hipLaunchKernelGGL((k_line2_apply<LM, true>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col); \
        else hipLaunchKernelGGL((k_line2_apply<LM, false>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col);        \
    } while (0)
    if (L.seg <= 8) VTK_LINE2_LAUNCH(8);
    else if (L.seg <= 16) VTK_LINE2_LAUNCH(16);
    else if (L.seg <= 25) VTK_LINE2_LAUNCH(25);
    else if (L.seg <= 32) VTK_LINE2_LAUNCH(32);
    else hipLaunchKernelGGL((k_line2_apply<0, false>), g, b, 0, s, L, D, t, z, v0, part0, part1, stop_col, col);
#undef VTK_LINE2_LAUNCH
    return hipGetLastError();
}

}  // namespace vtk
