// vtk_update.hip — gfx950 kernels of the value-update path (vtk_csr_update_values,
// vtk_csr_update_vlasov): an operator's sparsity pattern stays, its values change.
// Neither kernel reads or writes a column index, a dictionary or a code; both reproduce the
// creation path's values bit for bit (copies and the shared generator arithmetic only).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vtk_internal.hpp"
#include "vtk_vlasov.hpp"

namespace vtk {

// ---- SELL-64 values from the CSR values ------------------------------------------------------
// One wavefront per 64-row chunk q.  The chunk's CSR values are the contiguous span
// data[indptr[64q] .. indptr[min(64q + 64, n)]): the wave loads it coalesced into its own LDS
// stage, RF_STAGE entries at a time, and every lane copies its row's entries of the window to
// val + off[q] + lane, 64 entries apart (column-major, as k_sell_fill lays them out).  Entries
// k >= the row's length (and all of the rows past n) are the padding: zero.  A span within one
// window (every stencil operator: 64 rows x 5 or 9 entries) is read once and its k-th entries are
// written by all lanes together, 512 B per store; a longer span takes more windows, each lane
// then walking its own part of the window.
// No workgroup barrier: a wave's stage is its own, ordered by wave barriers.
constexpr int RF_STAGE = 1024;

template <typename VT>
__global__ __launch_bounds__(NT) void k_sell_refresh(const int32_t *__restrict__ indptr, const VT *__restrict__ data,
                                                     int64_t n, int64_t nch, const int64_t *__restrict__ off,
                                                     VT *__restrict__ val) {
    __shared__ VT stage[NT / 64][RF_STAGE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    VT *st = stage[wv];
    for (int64_t q = (int64_t)blockIdx.x * (NT / 64) + wv; q < nch; q += (int64_t)gridDim.x * (NT / 64)) {
        const int64_t r = q * 64 + lane, r1 = q * 64 + 64 < n ? q * 64 + 64 : n;
        const int64_t o = off[q];
        const int w = (int)((off[q + 1] - o) >> 6);
        const int64_t k0 = indptr[q * 64], k1 = indptr[r1];
        const int64_t rs = r < n ? indptr[r] : k1;
        const int len = r < n ? indptr[r + 1] - (int)rs : 0;
        VT *vv = val + o + lane;
        for (int k = len; k < w; ++k) vv[(int64_t)k * 64] = (VT)0;
        for (int64_t b = k0; b < k1; b += RF_STAGE) {
            const int cnt = (int)(k1 - b < RF_STAGE ? k1 - b : RF_STAGE);
            for (int i = lane; i < cnt; i += 64) st[i] = data[b + i];
            __builtin_amdgcn_wave_barrier();
            // the row's entries [ka, kb) lie in this window, at st[rs - b + k]
            const int64_t ka = b > rs ? b - rs : 0;
            const int64_t kb = b + cnt - rs < len ? b + cnt - rs : len;
            for (int64_t k = ka; k < kb; ++k) vv[k * 64] = st[rs - b + k];
            __builtin_amdgcn_wave_barrier();
        }
    }
}

hipError_t launch_sell_refresh(const int32_t *indptr, const void *data, int fp32, int64_t n, const int64_t *off,
                               void *val, hipStream_t s) {
    const int64_t nch = (n + 63) / 64;
    if (nch == 0) return hipSuccess;
    const int grid = (int)std::min<int64_t>((nch + NT / 64 - 1) / (NT / 64), 8192);
    if (fp32) hipLaunchKernelGGL(k_sell_refresh<float>, dim3(grid), dim3(NT), 0, s, indptr, (const float *)data, n, nch, off, (float *)val);
    else hipLaunchKernelGGL(k_sell_refresh<double>, dim3(grid), dim3(NT), 0, s, indptr, (const double *)data, n, nch, off, (double *)val);
    return hipGetLastError();
}

// ---- Vlasov values of rows [r0, r0 + nrows) ---------------------------------------------------
// The generator's row arithmetic is vlasov_row (vtk_vlasov.hpp), the one definition k_vlasov_fill
// and the host generator run: the values written here are theirs bit for bit, in the same
// (column-sorted) order.  The columns that vlasov_row also forms stay in registers.
template <typename VT>
__global__ __launch_bounds__(NT) void k_vlasov_values(vtk_vlasov_params p, int64_t r0, int64_t nrows,
                                                      const int32_t *__restrict__ indptr, VT *__restrict__ data) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * blockDim.x) {
        VlasovRow row;
        vlasov_row(p, r0 + i, row);
        const int32_t o = indptr[i];
        for (int k = 0; k < row.count; ++k) data[o + k] = (VT)row.val[k];
    }
}

hipError_t launch_vlasov_values(const vtk_vlasov_params &p, int64_t r0, int64_t nrows, const int32_t *indptr,
                                void *data, hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    if (p.fp32)
        hipLaunchKernelGGL(k_vlasov_values<float>, dim3(2048), dim3(NT), 0, s, p, r0, nrows, indptr,
                           static_cast<float *>(data));
    else
        hipLaunchKernelGGL(k_vlasov_values<double>, dim3(2048), dim3(NT), 0, s, p, r0, nrows, indptr,
                           static_cast<double *>(data));
    return hipGetLastError();
}

}  // namespace vtk
