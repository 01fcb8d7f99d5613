// vtk_bicgstab.hip — gfx950 kernels of the BiCGStab solver (vtk_bicgstab): the
// solver's own vector updates, their BJ-fused forms and the single-workgroup scalar step.  The two
// products of an iteration are launch_spmv (vtk_kernels.hip), the unfused preconditioner apply
// launch_bj_apply.  Across ranks k_bcg_reduce turns the partials a scalar step or k_bcg_x consumes
// into a small record (the sums and this rank's failure vote) that the driver all-reduces.
//
// Conventions of vtk_kernels.hip: fixed grid vector_grid(n) <= GMAX, one partial per workgroup and
// quantity (no float atomics), wave sums by DPP (block_sum), and every kernel returns at entry once
// *stop < tag (BicgState::stop, lowered by k_bcg_scalar).  -ffp-contract=off: the expressions below
// are SciPy's (scipy/sparse/linalg/_isolve/iterative.py, bicgstab), operation for operation.
//
// Element mapping: one row per lane, i = i0 + threadIdx.x with i0 uniform over the workgroup, in
// the plain and in the BJ-fused forms alike.  A block of bs <= 8 rows then sits in bs neighbouring
// lanes of one wavefront (i0 is a multiple of NT), so the fused forms take the block's other rows
// from registers; and since the mapping is the same, the partial sums of a fused launch equal the
// unfused launch's bit for bit.
#include "vtk_device.hpp"
#include "vtk_internal.hpp"

namespace vtk {

enum { BCG_PLAIN = 0, BCG_INV = 1, BCG_TRI = 2 };

// z_i = sum_j inv[i][j] y_{c0 + j}, j ascending from 0.0 (k_bj_apply's sum, the same bits): the
// block's y from the BS lanes holding it; lanes past n hold 0, as k_bj_apply reads them
template <int BS>
__device__ __forceinline__ double bj_inv_group(double y, bool act, int64_t row, int lane,
                                               const double *__restrict__ inv) {
    const int base = lane & ~(BS - 1);
    double m[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) m[j] = act ? inv[(size_t)row * BS + j] : 0.0;
    double z = 0.0;
#pragma unroll
    for (int j = 0; j < BS; ++j) z += m[j] * __shfl(y, base + j, 64);
    return z;
}

template <int MODE, int BS>
__device__ __forceinline__ double bcg_prec(double y, bool act, int64_t row, int lane, const double *mat, int64_t ld) {
    if constexpr (MODE == BCG_INV) return bj_inv_group<BS>(y, act, row, lane, mat);
    else return bj_tri_group<BS>(y, act, row, lane, mat, ld);
}

// p = r + beta (p - omega v) as SciPy forms it (p -= omega v; p *= beta; p += r); first: p = r.
// MODE != PLAIN: phat = M^-1 p in the same pass (mat: inverse rows, or the l | m | g factors)
template <int MODE, int BS>
__global__ __launch_bounds__(NT) void k_bcg_p(const BicgState *st, int first, int64_t n, const double *__restrict__ r,
                                              const double *__restrict__ v, double *__restrict__ p,
                                              double *__restrict__ phat, const double *__restrict__ mat, int64_t ld,
                                              const int *stop, int tag) {
    if (stopped(stop, tag)) return;
    const double beta = first ? 0.0 : st->beta, omega = first ? 0.0 : st->omega;
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * NT; i0 < n; i0 += (int64_t)gridDim.x * NT) {
        const int64_t i = i0 + threadIdx.x;
        const bool act = i < n;
        double pv = 0.0;
        if (act) {
            const double rv = r[i];
            if (first) {
                pv = rv;
            } else {
                pv = p[i] - omega * v[i];
                pv = pv * beta;
                pv = pv + rv;
            }
            // p is read again by the next k_bcg_p only (plain: by the apply or the SpMV first)
            if constexpr (MODE == BCG_PLAIN) p[i] = pv;
            else st_nt<2>(p + i, pv);
        }
        if constexpr (MODE != BCG_PLAIN) {
            const double z = bcg_prec<MODE, BS>(pv, act, i, lane, mat, ld);
            if (act) phat[i] = z;   // the SpMV gathers it next: a plain store
        }
    }
}

// s = r - alpha v in place, part[workgroup] = sum s^2; MODE != PLAIN: shat = M^-1 s in the same pass
template <int MODE, int BS>
__global__ __launch_bounds__(NT) void k_bcg_s(const BicgState *st, int64_t n, double *__restrict__ r,
                                              const double *__restrict__ v, double *__restrict__ shat,
                                              const double *__restrict__ mat, int64_t ld, double *part,
                                              const int *stop, int tag) {
    __shared__ double red[NT / 64];
    if (stopped(stop, tag)) return;
    const double alpha = st->alpha;
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int64_t i0 = (int64_t)blockIdx.x * NT; i0 < n; i0 += (int64_t)gridDim.x * NT) {
        const int64_t i = i0 + threadIdx.x;
        const bool act = i < n;
        double sv = 0.0;
        if (act) {
            sv = r[i] - alpha * v[i];
            r[i] = sv;
            acc += sv * sv;
        }
        if constexpr (MODE != BCG_PLAIN) {
            const double z = bcg_prec<MODE, BS>(sv, act, i, lane, mat, ld);
            if (act) shat[i] = z;
        }
    }
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// omega = <t, s> / <t, t> from the second product's partials (every workgroup sums them in the
// same fixed order, as k_bcg_scalar does after this kernel; across ranks: the two all-reduced sums
// of the omega record, and its vote); x += alpha phat; x += omega shat;
// r = s - omega t (s is r's buffer); part_rr = sum r^2, part_rho = sum rtilde r -- the next
// iteration's rho.  phat / shat may be p / s themselves (no preconditioner): no restrict on them
__global__ __launch_bounds__(NT) void k_bcg_x(const BicgState *st, Red ts, Red tt, int64_t n, double *x,
                                              const double *phat, const double *shat, double *r,
                                              const double *__restrict__ t, const double *__restrict__ rtilde,
                                              double *part_rr, double *part_rho, const double *vote, const int *stop,
                                              int tag) {
    __shared__ double red[NT / 64];
    if (stopped(stop, tag)) return;
    // across ranks: a rank voted failure in the omega all-reduce -- x and r stay as they are on every
    // rank (uniform: the record holds the same bits everywhere); scalar step C then lowers the flag
    if (vote != nullptr && *vote != 0.0) return;
    const double alpha = st->alpha;
    const double nts = reduce_red(ts, red);
    const double ntt = reduce_red(tt, red);
    const double omega = nts / ntt;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i0 = (int64_t)blockIdx.x * NT; i0 < n; i0 += (int64_t)gridDim.x * NT) {
        const int64_t i = i0 + threadIdx.x;
        if (i < n) {
            const double sh = shat[i];
            double xv = x[i] + alpha * phat[i];
            xv = xv + omega * sh;
            x[i] = xv;
            const double rv = r[i] - omega * ldnt(t + i);
            r[i] = rv;
            a0 += rv * rv;
            a1 += ldnt(rtilde + i) * rv;
        }
    }
    const double s0 = block_sum(a0, red);
    if (threadIdx.x == 0) part_rr[blockIdx.x] = s0;
    const double s1 = block_sum(a1, red);
    if (threadIdx.x == 0) part_rho[blockIdx.x] = s1;
}

// the half-step exit's update x += alpha phat: runs only when that exit lowered the flag to tag
__global__ __launch_bounds__(NT) void k_bcg_half_x(const BicgState *st, int64_t n, double *__restrict__ x,
                                                   const double *__restrict__ phat, const int *stop, int tag) {
    if (stop == nullptr || __builtin_nontemporal_load(stop) != tag) return;
    const double alpha = st->alpha;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
        x[i] = x[i] + alpha * phat[i];
}

// Scalar step: one workgroup sums the partials in fixed slot order (reduce_red) and lane 0 does
// SciPy's tests.  k: the iteration (loop index); phases
//   INIT  q0 = sum r^2 of the initial residual: the top tests of iteration 0 (rtilde = r: rho = q0)
//   A     q1 = <rtilde, v>: rv == 0 -> info -11; alpha = rho / rv
//   B     q0 = sum s^2: ||s|| < atol -> the half-step exit (k_bcg_half_x's tag)
//   C     q0 = <t, s>, q1 = <t, t>, q2 = sum r^2, q3 = <rtilde, r>: omega, then the top tests of
//         iteration k + 1 and its beta; last: the loop is exhausted instead, info = maxiter
// A stop lowers st->stop below every later tag and writes it through to the mapped host mirror.
// vote (across ranks): the failure-vote slot of the all-reduced record the q* come from.
__global__ __launch_bounds__(NT) void k_bcg_scalar(int phase, int64_t k, int last, int info_max, double atol, Red q0,
                                                   Red q1, Red q2, Red q3, const double *vote, BicgState *st,
                                                   int *stop_map, const int *stop, int tag) {
    __shared__ double red[NT / 64];
    if (stopped(stop, tag)) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (q0.p) s0 = reduce_red(q0, red);
    if (q1.p) s1 = reduce_red(q1, red);
    if (q2.p) s2 = reduce_red(q2, red);
    if (q3.p) s3 = reduce_red(q3, red);
    if (threadIdx.x != 0) return;
    const double tol2 = DBL_EPSILON * DBL_EPSILON;   // rhotol = omegatol = eps**2
    auto leave = [&](int info, int64_t iters, int stop_at) {
        st->info = info;
        st->iterations = iters;
        st->stop = stop_at;
        if (stop_map) __hip_atomic_store(stop_map, stop_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    // the tests at the top of iteration kk (its rho in rho_new), leaving at stop_at
    auto top = [&](int64_t kk, double rho_new, int stop_at) {
        if (st->rnorm < atol) return leave(0, kk, stop_at);
        st->rho_prev = st->rho;
        st->rho = rho_new;
        if (__builtin_fabs(rho_new) < tol2) return leave(-10, kk, stop_at);
        if (kk > 0) {
            if (__builtin_fabs(st->omega) < tol2) return leave(-11, kk, stop_at);
            st->beta = (rho_new / st->rho_prev) * (st->alpha / st->omega);
        }
    };
    // across ranks (q* all-reduced): a rank voted failure in this step's all-reduce -- every rank
    // reads the same sum, so every rank stops here, below each later tag of this iteration and
    // below the half-step tag (no x update follows); the host returns the error
    if (vote != nullptr && *vote != 0.0) {
        st->peer_failed = 1;
        const int at = phase == BCG_PH_INIT ? 0
                       : phase == BCG_PH_A  ? bcg_tag(k, 0)
                       : phase == BCG_PH_B  ? bcg_tag(k, 1)
                                            : bcg_tag(k, 3);
        return leave(0, k, at);
    }
    if (phase == BCG_PH_INIT) {
        st->rnorm = __builtin_sqrt(s0);
        top(0, s0, 0);
    } else if (phase == BCG_PH_A) {
        st->rv = s1;
        if (s1 == 0.0) return leave(-11, k, bcg_tag(k, 0));
        st->alpha = st->rho / s1;
    } else if (phase == BCG_PH_B) {
        st->snorm = __builtin_sqrt(s0);
        if (st->snorm < atol) {
            st->half_step = 1;
            return leave(0, k + 1, bcg_tag(k, 2));
        }
    } else {
        st->omega = s0 / s1;
        st->rnorm = __builtin_sqrt(s2);
        st->iterations = k + 1;
        if (last) return leave(info_max, k + 1, bcg_tag(k, 3));
        top(k + 1, s3, bcg_tag(k, 3));
    }
}

// Across ranks: this rank's partial sums of up to four quantities -> rec[0..nq), and this rank's
// sticky failure vote -> rec[nq]; the driver all-reduces rec (nq + 1 doubles) and the consumers read
// Red{rec + i, 1}.  One workgroup, the fixed slot order of reduce_red.
__global__ __launch_bounds__(NT) void k_bcg_reduce(Red q0, Red q1, Red q2, Red q3, int nq, const double *my_vote,
                                                   double *rec, const int *stop, int tag) {
    __shared__ double red[NT / 64];
    if (stopped(stop, tag)) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (nq > 0) s0 = reduce_red(q0, red);
    if (nq > 1) s1 = reduce_red(q1, red);
    if (nq > 2) s2 = reduce_red(q2, red);
    if (nq > 3) s3 = reduce_red(q3, red);
    if (threadIdx.x != 0) return;
    if (nq > 0) rec[0] = s0;
    if (nq > 1) rec[1] = s1;
    if (nq > 2) rec[2] = s2;
    if (nq > 3) rec[3] = s3;
    rec[nq] = *my_vote;
}

// ---- launchers ----------------------------------------------------------------------------------
static const double *bcg_mat(const BjOp &bj) { return bj.tri ? bj.tri : bj.inv; }

bool bcg_fusable(const BjOp &bj) {
    if (bj.bs < 1) return false;
    if (bj.tri) return bj.bs == 2 || bj.bs == 4 || bj.bs == 8;
    return bj.inv && (bj.bs == 1 || bj.bs == 2 || bj.bs == 4 || bj.bs == 8);
}

#define VTK_BCG_FUSED(KERNEL, ...)                                                                              \
    do {                                                                                                        \
        if (bj->tri) {                                                                                          \
            switch (bj->bs) {                                                                                   \
                case 2: hipLaunchKernelGGL((KERNEL<BCG_TRI, 2>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
                case 4: hipLaunchKernelGGL((KERNEL<BCG_TRI, 4>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
                default: hipLaunchKernelGGL((KERNEL<BCG_TRI, 8>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
            }                                                                                                   \
        } else {                                                                                                \
            switch (bj->bs) {                                                                                   \
                case 1: hipLaunchKernelGGL((KERNEL<BCG_INV, 1>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
                case 2: hipLaunchKernelGGL((KERNEL<BCG_INV, 2>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
                case 4: hipLaunchKernelGGL((KERNEL<BCG_INV, 4>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
                default: hipLaunchKernelGGL((KERNEL<BCG_INV, 8>), dim3(grid), dim3(NT), 0, s, __VA_ARGS__); break; \
            }                                                                                                   \
        }                                                                                                       \
    } while (0)

hipError_t launch_bcg_p(const BicgState *st, int first, int64_t n, const double *r, const double *v, double *p,
                        const BjOp *bj, double *phat, int grid, const int *stop, int tag, hipStream_t s) {
    if (bj) {
        if (!bcg_fusable(*bj) || !phat) return hipErrorInvalidValue;
        const double *mat = bcg_mat(*bj);
        const int64_t ld = bj->tri_ld;
        VTK_BCG_FUSED(k_bcg_p, st, first, n, r, v, p, phat, mat, ld, stop, tag);
    } else {
        hipLaunchKernelGGL((k_bcg_p<BCG_PLAIN, 1>), dim3(grid), dim3(NT), 0, s, st, first, n, r, v, p, (double *)nullptr,
                           (const double *)nullptr, (int64_t)0, stop, tag);
    }
    return hipGetLastError();
}

hipError_t launch_bcg_s(const BicgState *st, int64_t n, double *r, const double *v, const BjOp *bj, double *shat,
                        double *part, int grid, const int *stop, int tag, hipStream_t s) {
    if (bj) {
        if (!bcg_fusable(*bj) || !shat) return hipErrorInvalidValue;
        const double *mat = bcg_mat(*bj);
        const int64_t ld = bj->tri_ld;
        VTK_BCG_FUSED(k_bcg_s, st, n, r, v, shat, mat, ld, part, stop, tag);
    } else {
        hipLaunchKernelGGL((k_bcg_s<BCG_PLAIN, 1>), dim3(grid), dim3(NT), 0, s, st, n, r, v, (double *)nullptr,
                           (const double *)nullptr, (int64_t)0, part, stop, tag);
    }
    return hipGetLastError();
}
#undef VTK_BCG_FUSED

hipError_t launch_bcg_x(const BicgState *st, Red ts, Red tt, int64_t n, double *x, const double *phat,
                        const double *shat, double *r, const double *t, const double *rtilde, double *part_rr,
                        double *part_rho, const double *vote, int grid, const int *stop, int tag, hipStream_t s) {
    hipLaunchKernelGGL(k_bcg_x, dim3(grid), dim3(NT), 0, s, st, ts, tt, n, x, phat, shat, r, t, rtilde, part_rr,
                       part_rho, vote, stop, tag);
    return hipGetLastError();
}

hipError_t launch_bcg_half_x(const BicgState *st, int64_t n, double *x, const double *phat, int grid, const int *stop,
                             int tag, hipStream_t s) {
    hipLaunchKernelGGL(k_bcg_half_x, dim3(grid), dim3(NT), 0, s, st, n, x, phat, stop, tag);
    return hipGetLastError();
}

hipError_t launch_bcg_scalar(int phase, int64_t k, int last, int info_max, double atol, Red q0, Red q1, Red q2, Red q3,
                             const double *vote, BicgState *st, int *stop_map, const int *stop, int tag,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_bcg_scalar, dim3(1), dim3(NT), 0, s, phase, k, last, info_max, atol, q0, q1, q2, q3, vote,
                       st, stop_map, stop, tag);
    return hipGetLastError();
}

hipError_t launch_bcg_reduce(Red q0, Red q1, Red q2, Red q3, int nq, const double *my_vote, double *rec,
                             const int *stop, int tag, hipStream_t s) {
    if (nq < 0 || nq > 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcg_reduce, dim3(1), dim3(NT), 0, s, q0, q1, q2, q3, nq, my_vote, rec, stop, tag);
    return hipGetLastError();
}

}  // namespace vtk
