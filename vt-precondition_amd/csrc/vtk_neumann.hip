// vtk_neumann.hip -- vector kernels of the Neumann-series wrapper (vtk_neumann_create)
//
//   N_k^-1 r :  z_1 = M^-1 r ;  z_{i+1} = z_i + M^-1 (r - A z_i),  i = 1 .. k-1
//
// A correction is t = r - A z (launch_spmv's EPI_NEU_RESID), u = M^-1 t (the base's apply) and the
// addition w = z + u.  Bases with BJ-fused tiles run all three in one SpMV launch (EPI_NEU_CORR,
// vtk_kernels.hip); the line kinds store z + u from their last sweep (the ACC instantiations of
// k_line_apply, k_line2_apply and k_linec_correct); what is left -- block Jacobi without fused tiles,
// segments beyond the register sweeps -- adds here.  The last addition of an apply also leaves the
// partial sums its caller asked of the base's apply, or (k_neu_add_dc) the DCGS2 step's dots.
#include "vtk_internal.hpp"
#include "vtk_device.hpp"

namespace vtk {

// w = z + u: one addition per row, two rows per thread where the three vectors are 16-byte aligned
// (W = 2).  part0 = sum w^2, part1 = sum v0 w per workgroup (both optional).  w may alias z or u.
template <int W>
__global__ __launch_bounds__(NT) void k_neu_add(const double *z, const double *u, double *w, int64_t n,
                                                const double *__restrict__ v0, double *part0, double *part1,
                                                const int *stop_col, int col) {
    __shared__ double red[NT / 64];
    if (stopped(stop_col, col)) return;
    double acc0 = 0.0, acc1 = 0.0;
    const int64_t stride = (int64_t)W * gridDim.x * NT;
    for (int64_t i = (int64_t)W * ((int64_t)blockIdx.x * NT + threadIdx.x); i < n; i += stride) {
        if (W == 2 && i + 1 < n) {
            const double2 zv = ld_nt2<4>(z + i), uv = ld_nt2<4>(u + i);
            const double w0 = zv.x + uv.x, w1 = zv.y + uv.y;
            st_nt2<2>(w + i, w0, w1);
            acc0 += w0 * w0;
            acc0 += w1 * w1;
            if (v0) {
                acc1 += v0[i] * w0;
                acc1 += v0[i + 1] * w1;
            }
        } else {
            const double w0 = z[i] + u[i];
            w[i] = w0;
            acc0 += w0 * w0;
            if (v0) acc1 += v0[i] * w0;
        }
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

// the same addition as the head of k_dc_dots_rows: w = z + u is stored and stays in the thread's
// registers for the step's dots s = V_j^T p, zz = V_j^T w, |p|^2, p.w, |w|^2 (p = V[j]); row pairs per
// thread, every basis vector streamed once by 16-B non-temporal loads, JM >= j accumulators per
// quantity, the partials in launch_dc_dots' layout (part[q GMAX + block]).  z, u, w and V 16-byte
// aligned with an even leading dimension (the solver's workspace and the wrapper's vectors are)
template <int JM>
__global__ __launch_bounds__(NT) void k_neu_add_dc(const double *z, const double *u, double *w, int64_t n,
                                                   const double *__restrict__ V, int64_t ld, int j, double *part,
                                                   const int *stop_col, int col) {
    __shared__ double red[NT / 64][DC_NQ];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double *p = V + (size_t)j * ld;
    double as[JM], az[JM];
#pragma unroll
    for (int k = 0; k < JM; ++k) { as[k] = 0.0; az[k] = 0.0; }
    double aa = 0.0, ab = 0.0, ag = 0.0;
    const int64_t stride = 2 * (int64_t)gridDim.x * NT;
    for (int64_t i = 2 * ((int64_t)blockIdx.x * NT + threadIdx.x); i < n; i += stride) {
        const bool two = i + 1 < n;
        double2 pv, wv2;
        if (two) {
            pv = ld_nt2<4>(p + i);
            const double2 zv = ld_nt2<4>(z + i), uv = ld_nt2<4>(u + i);
            wv2 = make_double2(zv.x + uv.x, zv.y + uv.y);
            st_nt2<2>(w + i, wv2.x, wv2.y);
        } else {
            pv = make_double2(p[i], 0.0);
            wv2 = make_double2(z[i] + u[i], 0.0);
            w[i] = wv2.x;
        }
#pragma unroll
        for (int k = 0; k < JM; ++k) {
            if (k < j) {
                const double *vk = V + (size_t)k * ld + i;
                d2v v;
                if (two) v = ldnt2(vk);
                else { v.x = vk[0]; v.y = 0.0; }
                as[k] += v.x * pv.x;
                as[k] += v.y * pv.y;
                az[k] += v.x * wv2.x;
                az[k] += v.y * wv2.y;
            }
        }
        aa += pv.x * pv.x;
        aa += pv.y * pv.y;
        ab += pv.x * wv2.x;
        ab += pv.y * wv2.y;
        ag += wv2.x * wv2.x;
        ag += wv2.y * wv2.y;
    }
#pragma unroll
    for (int k = 0; k < JM; ++k) {
        if (k < j) {   // wave-uniform
            const double ts = wave_sum(as[k]), tz = wave_sum(az[k]);
            if (lane == 0) { red[wv][k] = ts; red[wv][DC_MAXJ + k] = tz; }
        }
    }
    {
        const double t0 = wave_sum(aa), t1 = wave_sum(ab), t2 = wave_sum(ag);
        if (lane == 0) { red[wv][2 * DC_MAXJ] = t0; red[wv][2 * DC_MAXJ + 1] = t1; red[wv][2 * DC_MAXJ + 2] = t2; }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < DC_NQ; q += NT) {
        const bool used = q < j || (q >= DC_MAXJ && q < DC_MAXJ + j) || q >= 2 * DC_MAXJ;
        if (used) {
            double t = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NT / 64; ++w2) t += red[w2][q];
            part[(size_t)q * GMAX + blockIdx.x] = t;
        }
    }
}

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t launch_neu_add(const double *z, const double *u, double *w, int64_t n, const double *v0, double *part0,
                          double *part1, int grid, const int *stop_col, int col, hipStream_t s) {
    if (n == 0 && part0 == nullptr) return hipSuccess;
    if (grid < 1 || (part0 && grid > GMAX)) return hipErrorInvalidValue;
    const dim3 g(grid), b(NT);
    if (aligned16(z) && aligned16(u) && aligned16(w))
        hipLaunchKernelGGL(k_neu_add<2>, g, b, 0, s, z, u, w, n, v0, part0, part1, stop_col, col);
    else
        hipLaunchKernelGGL(k_neu_add<1>, g, b, 0, s, z, u, w, n, v0, part0, part1, stop_col, col);
    return hipGetLastError();
}

hipError_t launch_neu_add_dc(const double *z, const double *u, double *w, int64_t n, const double *V, int64_t ld,
                             int j, double *part, int grid, const int *stop_col, int col, hipStream_t s) {
    if (j > DC_MAXJ || grid < 1 || grid > GMAX || (ld & 1) || !aligned16(z) || !aligned16(u) || !aligned16(w) || !aligned16(V))
        return hipErrorInvalidValue;
    const dim3 g(grid), b(NT);
    if (j <= 8) hipLaunchKernelGGL(k_neu_add_dc<8>, g, b, 0, s, z, u, w, n, V, ld, j, part, stop_col, col);
    else if (j <= 16) hipLaunchKernelGGL(k_neu_add_dc<16>, g, b, 0, s, z, u, w, n, V, ld, j, part, stop_col, col);
    else if (j <= 24) hipLaunchKernelGGL(k_neu_add_dc<24>, g, b, 0, s, z, u, w, n, V, ld, j, part, stop_col, col);
    else hipLaunchKernelGGL(k_neu_add_dc<DC_MAXJ>, g, b, 0, s, z, u, w, n, V, ld, j, part, stop_col, col);
    return hipGetLastError();
}

}  // namespace vtk
