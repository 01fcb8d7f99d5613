// vtk_cbasis.hip -- the compressed Krylov basis of vtk_gmres (vtk_gmres_set_basis VTK_BASIS_F32;
// DESIGN.md §3p): the DCGS2 split step's two basis passes, the cycle start and the x update with the
// finalised columns stored in float32 and every operation in float64.
//
//   Vc[k ld + i] = (float) v_k[i]     the finalised columns v^_0 .. v^_{m-1} (m + 1 columns of ld floats)
//   pa, pb                            two float64 vectors: the candidate p_j in the one of parity j,
//                                     p_{j+1} written to the other
//
// A column is rounded once, when the update pass (or the cycle start) stores it, and every later use
// -- the dots, the projections of the update pass, the x update -- widens the stored value: the
// arithmetic is k_dc_dots_rows', k_dc_update's, k_scale0's and k_xupdate's, in their order, with
// (double) Vc in place of V.  The step that stores v^_j already subtracts e_j v^_j, not e_j v_j, so
// the candidate p_{j+1} is w less its projection on the columns later steps will read.
//
// Every thread owns four consecutive rows: a column streams through 16-B non-temporal loads as the
// float64 kernels' do with two rows.  ld is a multiple of 64 and the workspace 64-B aligned, so
// Vc + k ld + 4 t is 16-B aligned and the float64 vectors' quads 32-B aligned.  The last quad of a
// vector whose length is no multiple of four takes the row-by-row path (rows past n read as zero and
// are never stored).
#include <algorithm>

#include "vtk_internal.hpp"
#include "vtk_device.hpp"

namespace vtk {

typedef float f4v __attribute__((ext_vector_type(4)));

struct Q4 {
    double v[4];
};

// rows i .. i + 3 of a float64 vector (full: all four below n)
__device__ __forceinline__ Q4 ld_q4(const double *__restrict__ p, int64_t i, int64_t n, bool full) {
    Q4 q;
    if (full) {
        const d2v a = ldnt2(p + i), b = ldnt2(p + i + 2);
        q.v[0] = a.x, q.v[1] = a.y, q.v[2] = b.x, q.v[3] = b.y;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) q.v[u] = i + u < n ? p[i + u] : 0.0;
    }
    return q;
}

// rows i .. i + 3 of a stored column, widened
__device__ __forceinline__ Q4 ld_q4f(const float *__restrict__ p, int64_t i, int64_t n, bool full) {
    Q4 q;
    if (full) {
        const f4v a = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(p + i));
        q.v[0] = (double)a.x, q.v[1] = (double)a.y, q.v[2] = (double)a.z, q.v[3] = (double)a.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) q.v[u] = i + u < n ? (double)p[i + u] : 0.0;
    }
    return q;
}

__device__ __forceinline__ void st_q4(double *__restrict__ p, int64_t i, int64_t n, bool full, const Q4 &q) {
    if (full) {
        st_nt2<2>(p + i, q.v[0], q.v[1]);
        st_nt2<2>(p + i + 2, q.v[2], q.v[3]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u < n) p[i + u] = q.v[u];
    }
}

// stores (float) q to the column and returns the stored values widened
__device__ __forceinline__ Q4 st_q4f(float *__restrict__ p, int64_t i, int64_t n, bool full, const Q4 &q) {
    const f4v f = {(float)q.v[0], (float)q.v[1], (float)q.v[2], (float)q.v[3]};
    if (full) {
        __builtin_nontemporal_store(f, reinterpret_cast<f4v *>(p + i));
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u < n) p[i + u] = f[u];
    }
    Q4 r;
#pragma unroll
    for (int u = 0; u < 4; ++u) r.v[u] = (double)f[u];
    return r;
}

#define CB_ROWS(i, n)                                                                                    \
    const int64_t stride_ = 4 * (int64_t)gridDim.x * NT;                                                 \
    for (int64_t i = 4 * ((int64_t)blockIdx.x * NT + threadIdx.x); i < (n); i += stride_)

// ------------------------------------------------------------------------------------------
// cycle start (k_scale0): v_0 = p * (1 / t), t = sqrt(reduce(p)); Vc[0] = (float) v_0 and the
// widened stored value back into the candidate buffer, so that step 0 applies the operator to v^_0
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_cb_scale0(Red p, double *__restrict__ p0, float *__restrict__ Vc,
                                                  int64_t n, double *S, int m, GmresState *st) {
    __shared__ double red[NT / 64];
    const double t = __builtin_sqrt(reduce_red(p, red));
    const double sc = 1.0 / t;
    CB_ROWS(i, n) {
        const bool full = i + 3 < n;
        Q4 v = ld_q4(p0, i, n, full);
#pragma unroll
        for (int u = 0; u < 4; ++u) v.v[u] = v.v[u] * sc;
        st_q4(p0, i, n, full, st_q4f(Vc, i, n, full, v));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int k = 0; k <= m; ++k) S[k] = 0.0;
        S[0] = t;
        st->stop_col = BIG_COL;
        st->breakdown = 0;
        st->xup_tag = -1;
    }
}

hipError_t launch_cb_scale0(Red p, double *p0, float *Vc, int64_t n, double *S, int m, GmresState *st, int grid,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_cb_scale0, dim3(grid), dim3(NT), 0, s, p, p0, Vc, n, S, m, st);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// the step's dots (k_dc_dots_rows): s = V^_j^T p, z = V^_j^T w, |p|^2, p.w, |w|^2 per workgroup in
// launch_dc_dots' layout (part[q GMAX + block]); w == null: s and |p|^2 only (the closing reduction)
// ------------------------------------------------------------------------------------------
template <int JM>
__global__ __launch_bounds__(NT) void k_cb_dots(const float *__restrict__ Vc, int64_t ld, int j,
                                                const double *__restrict__ p, const double *__restrict__ w,
                                                int64_t n, double *part, const int *stop_col, int col) {
    __shared__ double red[NT / 64][DC_NQ];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double as[JM], az[JM];
#pragma unroll
    for (int k = 0; k < JM; ++k) { as[k] = 0.0; az[k] = 0.0; }
    double aa = 0.0, ab = 0.0, ag = 0.0;
    CB_ROWS(i, n) {
        const bool full = i + 3 < n;
        const Q4 pv = ld_q4(p, i, n, full);
        Q4 wq{};
        if (w) wq = ld_q4(w, i, n, full);
#pragma unroll
        for (int k = 0; k < JM; ++k) {
            if (k < j) {
                const Q4 v = ld_q4f(Vc + (size_t)k * ld, i, n, full);
#pragma unroll
                for (int u = 0; u < 4; ++u) as[k] += v.v[u] * pv.v[u];
                if (w) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) az[k] += v.v[u] * wq.v[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) aa += pv.v[u] * pv.v[u];
        if (w) {
#pragma unroll
            for (int u = 0; u < 4; ++u) ab += pv.v[u] * wq.v[u];
#pragma unroll
            for (int u = 0; u < 4; ++u) ag += wq.v[u] * wq.v[u];
        }
    }
#pragma unroll
    for (int k = 0; k < JM; ++k) {
        if (k < j) {   // wave-uniform
            const double ts = wave_sum(as[k]);
            const double tz = w ? wave_sum(az[k]) : 0.0;
            if (lane == 0) { red[wv][k] = ts; red[wv][DC_MAXJ + k] = tz; }
        }
    }
    {
        const double t0 = wave_sum(aa), t1 = wave_sum(ab), t2 = wave_sum(ag);
        if (lane == 0) { red[wv][2 * DC_MAXJ] = t0; red[wv][2 * DC_MAXJ + 1] = t1; red[wv][2 * DC_MAXJ + 2] = t2; }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < DC_NQ; q += NT) {
        const bool used = q < j || (q >= DC_MAXJ && q < DC_MAXJ + j && w) || q == 2 * DC_MAXJ ||
                          (w && q > 2 * DC_MAXJ);
        if (used) {
            double t = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NT / 64; ++w2) t += red[w2][q];
            part[(size_t)q * GMAX + blockIdx.x] = t;
        }
    }
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t launch_cb_dots(const float *Vc, int64_t ld, int j, const double *p, const double *w, int64_t n,
                          double *part, int grid, const int *stop_col, int col, hipStream_t s) {
    if (j < 0 || j > DC_MAXJ || grid < 1 || grid > GMAX || (ld & 3) || !aligned16(Vc) || !aligned16(p) || !aligned16(w))
        return hipErrorInvalidValue;
    const dim3 g(grid), b(NT);
    if (j <= 8) hipLaunchKernelGGL(k_cb_dots<8>, g, b, 0, s, Vc, ld, j, p, w, n, part, stop_col, col);
    else if (j <= 16) hipLaunchKernelGGL(k_cb_dots<16>, g, b, 0, s, Vc, ld, j, p, w, n, part, stop_col, col);
    else if (j <= 24) hipLaunchKernelGGL(k_cb_dots<24>, g, b, 0, s, Vc, ld, j, p, w, n, part, stop_col, col);
    else hipLaunchKernelGGL(k_cb_dots<DC_MAXJ>, g, b, 0, s, Vc, ld, j, p, w, n, part, stop_col, col);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// the cycle's x update inside update pass j (dc_xupdate_body): x += sum_k y_k v^_k over the stored
// columns, y = H^-1 S at c = stop_col.  c == j: column j is not stored yet -- v_j = (p_j - V^_j s)
// rinv is formed as the pass would, rounded to float32 as the pass would store it, and enters x
// widened (j == 0: p_0 holds v^_0 already)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void cb_xupdate_body(const float *__restrict__ Vc, int64_t ld, int j, int c,
                                                const double *__restrict__ pj, int64_t n, const DcCoef *cf,
                                                double *__restrict__ x, const double *__restrict__ H,
                                                const double *__restrict__ S, int m) {
    __shared__ double ys[DC_MAXJ + 1], cs[DC_MAXJ];
    __shared__ double rinv_s;
    if (threadIdx.x == 0) {
        hess_solve(H, S, m, c, ys);
        rinv_s = cf->rinv;
    }
    if (c == j)
        for (int k = threadIdx.x; k < j; k += NT) cs[k] = cf->s[k];
    __syncthreads();
    const double rinv = rinv_s;
    const int kv = c == j ? j : c + 1;   // stored columns in the sum
    CB_ROWS(i, n) {
        const bool full = i + 3 < n;
        Q4 ax{}, a{};
        if (c == j) a = ld_q4(pj, i, n, full);
        for (int k = 0; k < kv; ++k) {
            const Q4 v = ld_q4f(Vc + (size_t)k * ld, i, n, full);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ax.v[u] += ys[k] * v.v[u];
                if (c == j) a.v[u] = a.v[u] - cs[k] * v.v[u];
            }
        }
        if (c == j) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double vj = j >= 1 ? a.v[u] * rinv : a.v[u];
                ax.v[u] += ys[j] * (double)(float)vj;
            }
        }
        if (full) {
            const double2 x0 = *reinterpret_cast<const double2 *>(x + i), x1 = *reinterpret_cast<const double2 *>(x + i + 2);
            st_wt(x + i, x0.x + ax.v[0]);
            st_wt(x + i + 1, x0.y + ax.v[1]);
            st_wt(x + i + 2, x1.x + ax.v[2]);
            st_wt(x + i + 3, x1.y + ax.v[3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + u < n) x[i + u] = x[i + u] + ax.v[u];
        }
    }
}

// ------------------------------------------------------------------------------------------
// update pass of step j (k_dc_update): a = p_j - sum_k s_k v^_k, t = w - sum_k e_k v^_k over the
// stored columns k < j; v_j = a rinv, Vc[j] = (float) v_j (j = 0: v^_0 is read from Vc[0]);
// t = t - e_j v^_j with the stored value widened; p_{j+1} = t q into pn, float64
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_cb_update(float *__restrict__ Vc, int64_t ld, int j,
                                                  const double *__restrict__ pj, const double *__restrict__ w,
                                                  double *__restrict__ pn, int64_t n, const DcCoef *cf,
                                                  const GmresState *st, double *x, const double *H, const double *S,
                                                  int m) {
    __shared__ double cs[DC_MAXJ], ce[DC_MAXJ + 1];
    __shared__ double rinv_s, q_s;
    if (__builtin_nontemporal_load(&st->xup_tag) == j) {   // the cycle's x update
        cb_xupdate_body(Vc, ld, j, __builtin_nontemporal_load(&st->stop_col), pj, n, cf, x, H, S, m);
        return;
    }
    if (stopped(&st->stop_col, j)) return;
    for (int k = threadIdx.x; k <= j; k += NT) {
        if (k < j) cs[k] = cf->s[k];
        ce[k] = cf->e[k];
    }
    if (threadIdx.x == 0) { rinv_s = cf->rinv; q_s = cf->q; }
    __syncthreads();
    const double rinv = rinv_s, q = q_s, ej = ce[j];
    float *vcj = Vc + (size_t)j * ld;
    CB_ROWS(i, n) {
        const bool full = i + 3 < n;
        Q4 a = ld_q4(pj, i, n, full), t = ld_q4(w, i, n, full);
        for (int k = 0; k < j; ++k) {
            const Q4 v = ld_q4f(Vc + (size_t)k * ld, i, n, full);
            const double sk = cs[k], ek = ce[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a.v[u] = a.v[u] - sk * v.v[u];
                t.v[u] = t.v[u] - ek * v.v[u];
            }
        }
        Q4 vh;
        if (j >= 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) a.v[u] = a.v[u] * rinv;
            vh = st_q4f(vcj, i, n, full, a);
        } else {
            vh = ld_q4f(vcj, i, n, full);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            t.v[u] = t.v[u] - ej * vh.v[u];
            t.v[u] = t.v[u] * q;
        }
        st_q4(pn, i, n, full, t);
    }
}

hipError_t launch_cb_update(float *Vc, int64_t ld, int j, const double *pj, const double *w, double *pn, int64_t n,
                            const DcCoef *cf, int grid, const GmresState *st, double *x, const double *H,
                            const double *S, int m, hipStream_t s) {
    if (j < 0 || j >= DC_MAXJ || grid < 1 || (ld & 3) || pj == pn || !aligned16(Vc) || !aligned16(pj) || !aligned16(w) ||
        !aligned16(pn) || !aligned16(x))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cb_update, dim3(grid), dim3(NT), 0, s, Vc, ld, j, pj, w, pn, n, cf, st, x, H, S, m);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// the host-enqueued x update at cycle end (k_xupdate): every column 0 .. col is stored
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_cb_xupdate(const double *__restrict__ H, const double *__restrict__ S,
                                                   const float *__restrict__ Vc, int64_t ld, double *__restrict__ x,
                                                   int64_t n, int m, const GmresState *st) {
    __shared__ double ys[DC_MAXJ + 1];
    if (st->xup_tag >= 0) return;   // an update pass did it
    const int col = st->stop_col < m ? st->stop_col : m - 1;
    if (threadIdx.x == 0) hess_solve(H, S, m, col, ys);
    __syncthreads();
    CB_ROWS(i, n) {
        const bool full = i + 3 < n;
        Q4 ax{};
        for (int k = 0; k <= col; ++k) {
            const Q4 v = ld_q4f(Vc + (size_t)k * ld, i, n, full);
#pragma unroll
            for (int u = 0; u < 4; ++u) ax.v[u] += ys[k] * v.v[u];
        }
        Q4 xv = ld_q4(x, i, n, full);
#pragma unroll
        for (int u = 0; u < 4; ++u) xv.v[u] = xv.v[u] + ax.v[u];
        st_q4(x, i, n, full, xv);
    }
}

hipError_t launch_cb_xupdate(const double *H, const double *S, const float *Vc, int64_t ld, double *x, int64_t n,
                             int m, const GmresState *st, int grid, hipStream_t s) {
    if (m < 1 || m > DC_MAXJ || grid < 1 || (ld & 3) || !aligned16(Vc) || !aligned16(x)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cb_xupdate, dim3(grid), dim3(NT), 0, s, H, S, Vc, ld, x, n, m, st);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// capture (vtk_gmres_capture): out[k ld + i] = (double) Vc[k ld + i] for the m + 1 columns, with the
// candidate still open at cycle end in its column jc = xup_tag (the update pass that became the x
// update left p_jc unstored), or m after a cycle that ran every update pass
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_cb_capture(const float *__restrict__ Vc, int64_t ld, int m,
                                                   const double *__restrict__ pa, const double *__restrict__ pb,
                                                   const GmresState *st, double *__restrict__ out) {
    const int tag = st->xup_tag;
    const int jc = tag >= 0 ? tag : m;
    const double *pc = (jc & 1) ? pb : pa;
    const int64_t total = (int64_t)(m + 1) * ld;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t k = e / ld, i = e - k * ld;
        out[e] = (k == jc && jc >= 1) ? pc[i] : (double)Vc[e];
    }
}

hipError_t launch_cb_capture(const float *Vc, int64_t ld, int m, const double *pa, const double *pb,
                             const GmresState *st, double *out, hipStream_t s) {
    const int64_t total = (int64_t)(m + 1) * ld;
    const int grid = (int)std::min<int64_t>(GMAX, (total + NT - 1) / NT);
    hipLaunchKernelGGL(k_cb_capture, dim3(grid), dim3(NT), 0, s, Vc, ld, m, pa, pb, st, out);
    return hipGetLastError();
}

}  // namespace vtk
