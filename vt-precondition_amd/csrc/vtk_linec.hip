// vtk_linec.hip — the periodic whole-line preconditioner (vtk_linecyclic_create).
//
// M keeps A's diagonal and the couplings between line neighbours modulo `period`: every
// (block, R mod stride) is one cyclic tridiagonal system of `period` unknowns, element i of it at
// index (block period + i) stride + j.  The solver is a recursive Schur complement on separators.
// A level cuts each line into segments of `seg` unknowns (the last may be shorter); the last
// unknown of a segment is its separator, the others its interior.  With T the interior's open
// tridiagonal matrix, a_f its first row's coupling to the separator on the left (cyclically, the
// previous segment's) and c_l its last row's coupling to the segment's own separator,
//     x_I = y - V xi - W eta,   y = T^-1 r_I,  V = T^-1 (a_f e_first),  W = T^-1 (c_l e_last),
// xi / eta the left / right separator values.  The separators of a line obey a cyclic tridiagonal
// system of one unknown per segment -- the next level, same layout, period = segments per line.
// The last level is one segment per line: its reduced system is the scalar pivot 1 / minv.
//
// Per level f = l | m | g | V | W (n doubles each).  Interior rows: the Thomas factors of T
// (k_line_setup's recurrences) and the spikes; separator rows: m = b_s, V = a_s, W = c_s, the
// row's own coefficients.  No pivoting.  Built with -ffp-contract=off; the operations per row are
// written out in DESIGN.md §3m.  Indices: every element index is < n < 2^31 by construction
// ((block period + i) stride + j with i < period, j < stride); lanes with j >= stride touch nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vtk_internal.hpp"
#include "vtk_device.hpp"

namespace vtk {

// a level as the kernels see it
struct LcView {
    double *f;
    int64_t n, S, P, seg, nseg, nblk, jb;
};

static LcView lc_view(const LineC &C, int lev) {
    const LineCLevel &v = C.lev[lev];
    return LcView{v.f, v.n, C.stride, v.period, v.seg, v.nseg, C.nblk, (C.stride + 63) / 64};
}

// wavefront item t -> (block, segment k, 64 consecutive j): the lane's segment
struct LcLane {
    int64_t base;    // element index of the segment's first unknown
    int64_t sidx;    // next-level index of the segment's separator
    int64_t left;    // next-level index of the separator on the left (the previous segment's)
    int64_t rbase;   // element index of the next segment's first unknown (cyclic)
    int64_t i0;      // line index of the first unknown
    int len, rlen;   // unknowns of this / the next segment (separator included)
    bool jv;
};
__device__ __forceinline__ LcLane lc_lane(const LcView &L, int64_t t, int lane) {
    const int64_t sk = t / L.jb, jw = t - sk * L.jb;
    const int64_t blk = sk / L.nseg, k = sk - blk * L.nseg;
    const int64_t j = jw * 64 + lane;
    const int64_t kl = k == 0 ? L.nseg - 1 : k - 1, kr = k + 1 == L.nseg ? 0 : k + 1;
    LcLane o;
    o.jv = j < L.S;
    o.i0 = k * L.seg;
    o.len = (int)(L.seg < L.P - o.i0 ? L.seg : L.P - o.i0);
    o.rlen = (int)(L.seg < L.P - kr * L.seg ? L.seg : L.P - kr * L.seg);
    o.base = (blk * L.P + o.i0) * L.S + j;
    o.rbase = (blk * L.P + kr * L.seg) * L.S + j;
    o.sidx = sk * L.S + j;
    o.left = (blk * L.nseg + kl) * L.S + j;
    return o;
}

// ---- setup -------------------------------------------------------------------------------------
// row r's coefficients: b = the stored entries with col == row, a / c those at the left / right
// line neighbour cl / cr, each summed in stored order from 0.0 in double (k_line_setup's b)
struct LcCoef {
    double a, b, c;
};
template <typename VT>
__device__ __forceinline__ LcCoef lc_coef(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                          const VT *__restrict__ data, const double *__restrict__ co, int64_t n,
                                          int64_t r, int64_t cl, int64_t cr) {
    if (co) return LcCoef{co[r], co[n + r], co[2 * n + r]};
    double a = 0.0, b = 0.0, c = 0.0;
    for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k) {
        const int64_t col = indices[k];
        const double v = (double)data[k];
        b = col == r ? b + v : b;
        a = col == cl ? a + v : a;
        c = col == cr ? c + v : c;
    }
    return LcCoef{a, b, c};
}

// factors and spikes of the lane's segment.  co == null: level 0, coefficients from the CSR (local
// columns: every cyclic line lies on this rank); else the level's a | b | c written by
// k_linec_reduce.  bad: the smallest element index of this level with a zero or non-finite pivot.
// open (level 0 of lines that span the ranks): the line's chunk is an open system,
// the first row's a and the last row's c are zero whatever the CSR stores at those columns
template <typename VT>
__global__ __launch_bounds__(NT) void k_linec_setup(LcView L, const int32_t *__restrict__ indptr,
                                                    const int32_t *__restrict__ indices,
                                                    const VT *__restrict__ data, const double *__restrict__ co,
                                                    unsigned long long *bad, int open) {
    const int lane = threadIdx.x & 63;
    const int64_t t = ((int64_t)blockIdx.x * NT + threadIdx.x) >> 6;
    if (t >= L.nblk * L.nseg * L.jb) return;
    const LcLane q = lc_lane(L, t, lane);
    if (!q.jv) return;
    const int64_t S = L.S, n = L.n, wrap = (L.P - 1) * S;
    double *l = L.f, *m = L.f + n, *g = L.f + 2 * n, *V = L.f + 3 * n, *W = L.f + 4 * n;
    const int nq = q.len - 1;
    double mp = 0.0, cp = 0.0, dp = 0.0;
    for (int u = 0; u < nq; ++u) {
        const int64_t r = q.base + (int64_t)u * S, i = q.i0 + u;
        const LcCoef k3 = lc_coef(indptr, indices, data, co, n, r, i == 0 ? r + wrap : r - S, i == L.P - 1 ? r - wrap : r + S);
        const double a = open && i == 0 ? 0.0 : k3.a, b = k3.b, c = k3.c;   // (the last row is a separator)
        double lv = 0.0, uv, dv;
        if (u > 0) {
            lv = a * mp;
            uv = b - lv * cp;
            dv = -(lv * dp);
        } else {
            uv = b;
            dv = a;
        }
        const double mv = 1.0 / uv;
        if (uv == 0.0 || !isfinite(uv) || !isfinite(mv)) atomicMin(bad, (unsigned long long)r);
        l[r] = lv;
        m[r] = mv;
        g[r] = u + 1 < nq ? c * mv : 0.0;
        V[r] = dv;   // the forward sweep of V's right-hand side; the backward sweep below finishes it
        mp = mv;
        cp = c;
        dp = dv;
    }
    {   // the separator's own row
        const int64_t r = q.base + (int64_t)nq * S, i = q.i0 + nq;
        const LcCoef k3 = lc_coef(indptr, indices, data, co, n, r, i == 0 ? r + wrap : r - S, i == L.P - 1 ? r - wrap : r + S);
        l[r] = 0.0;
        m[r] = k3.b;
        g[r] = 0.0;
        V[r] = open && i == 0 ? 0.0 : k3.a;
        W[r] = open && i == L.P - 1 ? 0.0 : k3.c;
    }
    double vn = 0.0, wn = 0.0;
    for (int u = nq - 1; u >= 0; --u) {
        const int64_t r = q.base + (int64_t)u * S;
        const double mv = m[r], gv = g[r];
        const double vv = mv * V[r] - gv * vn;
        const double wv = u == nq - 1 ? mv * cp : -(gv * wn);   // cp: the last interior row's c
        V[r] = vv;
        W[r] = wv;
        vn = vv;
        wn = wv;
    }
}

// the separators' system: a' | b' | c' of the next level (co_out, n1 doubles each), or -- the last
// level, one segment per line -- minv = 1 / ((b' + a') + c')
__global__ __launch_bounds__(NT) void k_linec_reduce(LcView L, double *__restrict__ co_out, int64_t n1,
                                                     double *__restrict__ minv, unsigned long long *bad) {
    const int lane = threadIdx.x & 63;
    const int64_t t = ((int64_t)blockIdx.x * NT + threadIdx.x) >> 6;
    if (t >= L.nblk * L.nseg * L.jb) return;
    const LcLane q = lc_lane(L, t, lane);
    if (!q.jv) return;
    const int64_t S = L.S, n = L.n;
    const double *m = L.f + n, *V = L.f + 3 * n, *W = L.f + 4 * n;
    const int64_t s = q.base + (int64_t)(q.len - 1) * S;
    const double as = V[s], cs = W[s];
    double ap = as, bb = m[s], cq = cs;
    if (q.len > 1) {
        ap = -(as * V[s - S]);
        bb = bb - as * W[s - S];
    }
    if (q.rlen > 1) {
        cq = -(cs * W[q.rbase]);
        bb = bb - cs * V[q.rbase];
    }
    if (minv) {
        const double piv = (bb + ap) + cq;
        const double mv = 1.0 / piv;
        if (piv == 0.0 || !isfinite(piv) || !isfinite(mv)) atomicMin(bad, (unsigned long long)q.sidx);
        minv[q.sidx] = mv;
    } else {
        co_out[q.sidx] = ap;
        co_out[n1 + q.sidx] = bb;
        co_out[2 * n1 + q.sidx] = cq;
    }
}

// ---- apply -------------------------------------------------------------------------------------
// phase 1 of a level: y = T^-1 r on the lane's interior rows (forward d = r - l d_prev, backward
// y = m d - g y_next), written to z; separator rows are left alone.  LQ > 0: the lane's rows in
// registers, every load issued before the recurrence (addresses clamped to element 0 past the
// interior, results discarded).  LQ == 0: d goes through z.  r and z may alias.
template <int LQ>
__global__ __launch_bounds__(NT) void k_linec_sweep(LcView L, const double *r, double *z, const int *stop_col,
                                                    int col) {
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.nseg * L.jb, S = L.S;
    const double *l = L.f, *m = L.f + L.n, *g = L.f + 2 * L.n;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        const int nq = q.jv ? q.len - 1 : 0;
        if constexpr (LQ > 0) {
            double e[LQ], gg[LQ];
            double dp = 0.0;
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                const bool ok = u < nq;
                const int k = ok ? (int)(q.base + (int64_t)u * S) : 0;
                const double mv = ld_nt<8>(m + k), lv = ld_nt<8>(l + k), gv = ld_nt<8>(g + k);
                const double dv = ld_nt<8>(r + k) - lv * dp;
                e[u] = mv * dv;
                gg[u] = gv;
                if (ok) dp = dv;
            }
            double zn = 0.0;
#pragma unroll
            for (int u = LQ - 1; u >= 0; --u) {
                const double zv = e[u] - gg[u] * zn;
                if (u < nq) {
                    st_nt<4>(z + (int)(q.base + (int64_t)u * S), zv);
                    zn = zv;
                }
            }
        } else {
            double dp = 0.0;
            for (int u = 0; u < nq; ++u) {
                const int64_t k = q.base + (int64_t)u * S;
                const double dv = r[k] - l[k] * dp;
                z[k] = dv;
                dp = dv;
            }
            double zn = 0.0;
            for (int u = nq - 1; u >= 0; --u) {
                const int64_t k = q.base + (int64_t)u * S;
                const double zv = m[k] * z[k] - g[k] * zn;
                z[k] = zv;
                zn = zv;
            }
        }
    }
}

// phase 2, first part: the separators' right-hand sides, one lane per separator:
// xr = (r_s - a_s y_before) - c_s y_after, y from z (a neighbour that is itself a separator has
// its term in the reduced matrix instead)
__global__ __launch_bounds__(NT) void k_linec_gather(LcView L, const double *r, const double *z,
                                                     double *__restrict__ xr, const int *stop_col, int col) {
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.nseg * L.jb, S = L.S;
    const double *V = L.f + 3 * L.n, *W = L.f + 4 * L.n;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        if (!q.jv) continue;
        const int64_t s = q.base + (int64_t)(q.len - 1) * S;
        double rr = r[s];
        if (q.len > 1) rr = rr - V[s] * z[s - S];
        if (q.rlen > 1) rr = rr - W[s] * z[q.rbase];
        xr[q.sidx] = rr;
    }
}

// the last level, one lane per line: the sweep, the scalar reduced system sigma = rr minv, the
// correction -- all through x (in place; a lane's rows are its own).  The walk is latency-bound
// (one lane per line, every step behind the one before): each pass loads its operands LCB rows at a
// time, all in flight before the first of their recurrence steps
constexpr int LCB = 8;
__global__ __launch_bounds__(NT) void k_linec_serial(LcView L, double *x, const double *__restrict__ minv,
                                                     const int *stop_col, int col) {
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.jb, S = L.S;
    const double *__restrict__ l = L.f, *__restrict__ m = L.f + L.n, *__restrict__ g = L.f + 2 * L.n;
    const double *__restrict__ V = L.f + 3 * L.n, *__restrict__ W = L.f + 4 * L.n;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        if (!q.jv) continue;
        const int nq = q.len - 1;
        double p0[LCB], p1[LCB], p2[LCB];
        double dp = 0.0;
        for (int u0 = 0; u0 < nq; u0 += LCB) {
#pragma unroll
            for (int i = 0; i < LCB; ++i) {
                const int64_t k = q.base + (int64_t)(u0 + i < nq ? u0 + i : u0) * S;
                p0[i] = x[k];
                p1[i] = l[k];
            }
#pragma unroll
            for (int i = 0; i < LCB; ++i) {
                if (u0 + i < nq) {
                    const double dv = p0[i] - p1[i] * dp;
                    x[q.base + (int64_t)(u0 + i) * S] = dv;
                    dp = dv;
                }
            }
        }
        double zn = 0.0;
        for (int u0 = nq - 1; u0 >= 0; u0 -= LCB) {
#pragma unroll
            for (int i = 0; i < LCB; ++i) {
                const int64_t k = q.base + (int64_t)(u0 - i >= 0 ? u0 - i : u0) * S;
                p0[i] = x[k];
                p1[i] = m[k];
                p2[i] = g[k];
            }
#pragma unroll
            for (int i = 0; i < LCB; ++i) {
                if (u0 - i >= 0) {
                    const double zv = p1[i] * p0[i] - p2[i] * zn;
                    x[q.base + (int64_t)(u0 - i) * S] = zv;
                    zn = zv;
                }
            }
        }
        const int64_t s = q.base + (int64_t)nq * S;
        double rr = x[s];
        if (nq > 0) {
            rr = rr - V[s] * x[s - S];
            rr = rr - W[s] * x[q.base];
        }
        const double sig = rr * minv[q.sidx];
        for (int u0 = 0; u0 < nq; u0 += LCB) {
#pragma unroll
            for (int i = 0; i < LCB; ++i) {
                const int64_t k = q.base + (int64_t)(u0 + i < nq ? u0 + i : u0) * S;
                p0[i] = x[k];
                p1[i] = V[k];
                p2[i] = W[k];
            }
#pragma unroll
            for (int i = 0; i < LCB; ++i)
                if (u0 + i < nq) x[q.base + (int64_t)(u0 + i) * S] = (p0[i] - p1[i] * sig) - p2[i] * sig;
        }
        x[s] = sig;
    }
}

// phase 3 of a level: z = (y - V xi) - W eta on the interior rows, z = eta on the separator's;
// xs the next level's solution.  part0 = sum z^2, part1 = sum v0 z (optional) per workgroup
template <int LQ>
__global__ __launch_bounds__(NT) void k_linec_correct(LcView L, double *z, const double *__restrict__ xs,
                                                      const double *__restrict__ v0, double *part0, double *part1,
                                                      const int *stop_col, int col) {
    __shared__ double red[NT / 64];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.nseg * L.jb, S = L.S;
    const double *V = L.f + 3 * L.n, *W = L.f + 4 * L.n;
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        if (!q.jv) continue;
        const int nq = q.len - 1;
        const double xi = xs[q.left], eta = xs[q.sidx];
        if constexpr (LQ > 0) {
            double y[LQ], vv[LQ], ww[LQ];
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                const int k = u < nq ? (int)(q.base + (int64_t)u * S) : 0;
                y[u] = ld_nt<8>(z + k);
                vv[u] = ld_nt<8>(V + k);
                ww[u] = ld_nt<8>(W + k);
            }
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                if (u < nq) {
                    const int k = (int)(q.base + (int64_t)u * S);
                    const double zv = (y[u] - vv[u] * xi) - ww[u] * eta;
                    st_nt<4>(z + k, zv);
                    acc0 += zv * zv;
                    if (v0) acc1 += v0[k] * zv;
                }
            }
        } else {
            for (int u = 0; u < nq; ++u) {
                const int64_t k = q.base + (int64_t)u * S;
                const double zv = (z[k] - V[k] * xi) - W[k] * eta;
                z[k] = zv;
                acc0 += zv * zv;
                if (v0) acc1 += v0[k] * zv;
            }
        }
        const int64_t s = q.base + (int64_t)nq * S;
        z[s] = eta;
        acc0 += eta * eta;
        if (v0) acc1 += v0[s] * eta;
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

// the same pass storing acc + z (level 0 only; the Neumann wrapper's correction): one
// more addition per row, the partials those of the stored sum.  z must not alias acc.  (A kernel
// of its own: k_linec_correct keeps its code.)
template <int LQ>
__global__ __launch_bounds__(NT) void k_linec_correct_acc(LcView L, double *z, const double *__restrict__ xs,
                                                          const double *__restrict__ v0, double *part0, double *part1,
                                                          const int *stop_col, int col, const double *__restrict__ acc) {
    __shared__ double red[NT / 64];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.nseg * L.jb, S = L.S;
    const double *V = L.f + 3 * L.n, *W = L.f + 4 * L.n;
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        if (!q.jv) continue;
        const int nq = q.len - 1;
        const double xi = xs[q.left], eta = xs[q.sidx];
        if constexpr (LQ > 0) {
            double y[LQ], vv[LQ], ww[LQ];
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                const int k = u < nq ? (int)(q.base + (int64_t)u * S) : 0;
                y[u] = ld_nt<8>(z + k);
                vv[u] = ld_nt<8>(V + k);
                ww[u] = ld_nt<8>(W + k);
            }
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                if (u < nq) {
                    const int k = (int)(q.base + (int64_t)u * S);
                    const double zv = acc[k] + ((y[u] - vv[u] * xi) - ww[u] * eta);
                    st_nt<4>(z + k, zv);
                    acc0 += zv * zv;
                    if (v0) acc1 += v0[k] * zv;
                }
            }
        } else {
            for (int u = 0; u < nq; ++u) {
                const int64_t k = q.base + (int64_t)u * S;
                const double zv = acc[k] + ((z[k] - V[k] * xi) - W[k] * eta);
                z[k] = zv;
                acc0 += zv * zv;
                if (v0) acc1 += v0[k] * zv;
            }
        }
        const int64_t s = q.base + (int64_t)nq * S;
        const double zs = acc[s] + eta;
        z[s] = zs;
        acc0 += zs * zs;
        if (v0) acc1 += v0[s] * zs;
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

// ---- lines that span the ranks: the rank level -----------------------------------
// The levels above solve the rank's open chunk M_p of every line (one block, period = P_p).  With
// V_p = M_p^-1 (a_first e_first), W_p = M_p^-1 (c_last e_last), xi the previous rank's last unknown
// and eta the next rank's first,  x_p = y_p - V_p xi - W_p eta.  The kernels below: one lane per
// line j, 64 consecutive j per wavefront, every table [..][stride] (coalesced).

// rhs[row] = the row's stored entries at column ecol[j], summed in stored order from 0.0; the row
// is the line's first local one (which 0: a_first) or its last (which 1: c_last).  rhs is zero elsewhere
template <typename VT>
__global__ __launch_bounds__(NT) void k_linec_span_rhs(int64_t S, int64_t P, const int32_t *__restrict__ indptr,
                                                       const int32_t *__restrict__ indices, const VT *__restrict__ data,
                                                       const int32_t *__restrict__ ecol, int which, double *rhs) {
    const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= S) return;
    const int64_t r = which ? (P - 1) * S + j : j;
    const int32_t cc = ecol[which * S + j];
    double a = 0.0;
    if (cc >= 0)
        for (int32_t k = indptr[r]; k < indptr[r + 1]; ++k) a = indices[k] == cc ? a + (double)data[k] : a;
    rhs[r] = a;
}

// the four tips of the rank's spikes: V_first | V_last | W_first | W_last
__global__ __launch_bounds__(NT) void k_linec_span_tips(int64_t S, int64_t P, int64_t n, const double *__restrict__ vw,
                                                        double *__restrict__ tsend) {
    const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= S) return;
    const int64_t last = (P - 1) * S + j;
    tsend[j] = vw[j];
    tsend[S + j] = vw[last];
    tsend[2 * S + j] = vw[n + j];
    tsend[3 * S + j] = vw[n + last];
}

// the chunk's two edge values after phases 0 and 1: y_last is the last segment's separator value
// (level 1's solution), y_first the level-0 correction of the first row, (y - V xi0) - W eta0
__global__ __launch_bounds__(NT) void k_linec_span_edge(LcView L, const double *__restrict__ z,
                                                        const double *__restrict__ xs, double *__restrict__ edge,
                                                        const int *stop_col, int col) {
    if (stopped(stop_col, col)) return;
    const int64_t S = L.S, j = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= S) return;
    const double *V = L.f + 3 * L.n, *W = L.f + 4 * L.n;
    const double xi0 = xs[(L.nseg - 1) * S + j], eta0 = xs[j];
    edge[j] = (z[j] - V[j] * xi0) - W[j] * eta0;
    edge[S + j] = xi0;
}

// The interface system of line j.  Rank p's first and last unknowns f_p, l_p obey
//     f_p + Vf_p l_{p-1} + Wf_p f_{p+1} = yf_p,     l_p + Vl_p l_{p-1} + Wl_p f_{p+1} = yl_p
// (indices modulo W).  Elimination from rank 0 on, no pivoting: the chunks 0..p-1 merged into one
// have the same form, (F, L) = (Yf, Yl) - (AVf, AVl) xi - (AWf, AWl) f_p with F = f_0, L = l_{p-1}
// and xi = l_{W-1}; its last equation and rank p's first give, with d = 1 / (1 - Vf_p AWl),
//     f_p = fa + fb xi + fc f_{p+1},   fa = d (yf_p - Vf_p Yl), fb = d (Vf_p AVl), fc = -(d Wf_p),
//     l_{p-1} = la - lb xi - lc f_p,   (la, lb, lc) = (Yl, AVl, AWl) before the merge.
// After rank W-1 the cycle closes, xi = L and f_W = F:
//     F (1 + AWf) + L AVf = Yf,   F AWl + L (1 + AVl) = Yl        (world 1: exactly this)
// solved by Cramer's rule; then f_p, l_{p-1} backwards.  This rank keeps xi = l_{me-1} and
// eta = f_{me+1}.  The per-rank coefficients live in registers (WM >= W, loops unrolled).
// bad (setup): the smallest j with a zero or non-finite d or determinant
template <int WM>
__global__ __launch_bounds__(NT) void k_linec_span_iface(int64_t S, int W, int me, const double *__restrict__ tips,
                                                         const double *__restrict__ edges, double *__restrict__ xe,
                                                         unsigned long long *bad, const int *stop_col, int col) {
    if (stopped(stop_col, col)) return;
    const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (j >= S) return;
    const int64_t tq = 4 * S + 1, eq = 2 * S;
    double fa[WM], fb[WM], fc[WM], la[WM], lb[WM], lc[WM];
    double Yf = edges[j], Yl = edges[S + j];
    double AVf = tips[j], AVl = tips[S + j], AWf = tips[2 * S + j], AWl = tips[3 * S + j];
    bool ok = true;
#pragma unroll
    for (int p = 1; p < WM; ++p) {
        if (p < W) {
            const double *t = tips + (int64_t)p * tq, *e = edges + (int64_t)p * eq;
            const double Vf = t[j], Vl = t[S + j], Wf = t[2 * S + j], Wl = t[3 * S + j];
            const double yf = e[j], yl = e[S + j];
            const double piv = 1.0 - Vf * AWl;
            const double d = 1.0 / piv;
            ok = ok && piv != 0.0 && isfinite(piv) && isfinite(d);
            fa[p] = d * (yf - Vf * Yl);
            fb[p] = d * (Vf * AVl);
            fc[p] = -(d * Wf);
            la[p] = Yl;
            lb[p] = AVl;
            lc[p] = AWl;
            // F = Yf - AVf xi - AWf f_p with f_p substituted
            Yf = Yf - AWf * fa[p];
            AVf = AVf + AWf * fb[p];
            AWf = AWf * fc[p];
            // l_{p-1} = qa - qb xi - qc f_{p+1}, then l_p = yl - Vl l_{p-1} - Wl f_{p+1}
            const double qa = la[p] - lc[p] * fa[p], qb = lb[p] + lc[p] * fb[p], qc = lc[p] * fc[p];
            Yl = yl - Vl * qa;
            AVl = -(Vl * qb);
            AWl = Wl - Vl * qc;
        }
    }
    const double m00 = 1.0 + AWf, m11 = 1.0 + AVl;
    const double det = m00 * m11 - AVf * AWl;
    const double di = 1.0 / det;
    ok = ok && det != 0.0 && isfinite(det) && isfinite(di);
    if (bad && !ok) atomicMin(bad, (unsigned long long)j);
    const double F = (Yf * m11 - AVf * Yl) * di, Ll = (m00 * Yl - AWl * Yf) * di;
    double eta = F, xi_me = Ll, eta_me = F;
#pragma unroll
    for (int p = WM - 1; p >= 1; --p) {
        if (p < W) {
            const double fp = (fa[p] + fb[p] * Ll) + fc[p] * eta;
            const double lp = (la[p] - lb[p] * Ll) - lc[p] * fp;   // l_{p-1}
            if (p == me) {
                xi_me = lp;
                eta_me = eta;
            }
            eta = fp;
        }
    }
    if (me == 0) eta_me = eta;   // f_1 (world 1: f_0 itself)
    xe[j] = xi_me;
    xe[S + j] = eta_me;
}

// phase 3 with the rank terms fused in (k_linec_correct keeps its code): interior rows
// z = (((y - V xi0) - W eta0) - V_p xi) - W_p eta, separator rows z = (eta0 - V_p xi) - W_p eta;
// xi0 / eta0 the level's separator values (xs), xi / eta the rank's (xe).  The partials are
// k_linec_correct's
template <int LQ>
__global__ __launch_bounds__(NT) void k_linec_correct_span(LcView L, double *z, const double *__restrict__ xs,
                                                           const double *__restrict__ vw, const double *__restrict__ xe,
                                                           const double *__restrict__ v0, double *part0, double *part1,
                                                           const int *stop_col, int col) {
    __shared__ double red[NT / 64];
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t nitems = L.nblk * L.nseg * L.jb, S = L.S;
    const double *V = L.f + 3 * L.n, *W = L.f + 4 * L.n, *VP = vw, *WP = vw + L.n;
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * (NT / 64) + wv; t < nitems; t += (int64_t)gridDim.x * (NT / 64)) {
        const LcLane q = lc_lane(L, t, lane);
        if (!q.jv) continue;
        const int nq = q.len - 1;
        const int64_t j = (t % L.jb) * 64 + lane;
        const double xi0 = xs[q.left], eta0 = xs[q.sidx], xi = xe[j], eta = xe[S + j];
        if constexpr (LQ > 0) {
            // y, V, W in registers as in k_linec_correct; V_p and W_p are loaded row by row behind
            // them (all five held at once took 320 registers at LQ 24, one wave per SIMD; this
            // form 225, two waves as k_linec_correct<24>)
            double y[LQ], vv[LQ], ww[LQ];
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                const int k = u < nq ? (int)(q.base + (int64_t)u * S) : 0;
                y[u] = ld_nt<8>(z + k);
                vv[u] = ld_nt<8>(V + k);
                ww[u] = ld_nt<8>(W + k);
            }
#pragma unroll
            for (int u = 0; u < LQ; ++u) {
                if (u < nq) {
                    const int k = (int)(q.base + (int64_t)u * S);
                    const double zv = (((y[u] - vv[u] * xi0) - ww[u] * eta0) - ld_nt<8>(VP + k) * xi) - ld_nt<8>(WP + k) * eta;
                    st_nt<4>(z + k, zv);
                    acc0 += zv * zv;
                    if (v0) acc1 += v0[k] * zv;
                }
            }
        } else {
            for (int u = 0; u < nq; ++u) {
                const int64_t k = q.base + (int64_t)u * S;
                const double zv = (((z[k] - V[k] * xi0) - W[k] * eta0) - VP[k] * xi) - WP[k] * eta;
                z[k] = zv;
                acc0 += zv * zv;
                if (v0) acc1 += v0[k] * zv;
            }
        }
        const int64_t s = q.base + (int64_t)nq * S;
        const double zs = (eta0 - VP[s] * xi) - WP[s] * eta;
        z[s] = zs;
        acc0 += zs * zs;
        if (v0) acc1 += v0[s] * zs;
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

// ---- launchers ---------------------------------------------------------------------------------
static int lc_grid(const LcView &L, int cap) {
    const int64_t items = L.nblk * L.nseg * L.jb;
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + NT / 64 - 1) / (NT / 64), cap));
}
constexpr int LC_CAP = 8 * GMAX;   // workgroups of a non-reducing launch

static void lc_sweep(const LcView &L, const double *r, double *z, const int *stop_col, int col, hipStream_t s) {
    const dim3 g(lc_grid(L, LC_CAP)), b(NT);
    if (L.seg <= 8) hipLaunchKernelGGL(k_linec_sweep<7>, g, b, 0, s, L, r, z, stop_col, col);
    else if (L.seg <= 16) hipLaunchKernelGGL(k_linec_sweep<15>, g, b, 0, s, L, r, z, stop_col, col);
    else if (L.seg <= 25) hipLaunchKernelGGL(k_linec_sweep<24>, g, b, 0, s, L, r, z, stop_col, col);
    else if (L.seg <= 32) hipLaunchKernelGGL(k_linec_sweep<31>, g, b, 0, s, L, r, z, stop_col, col);
    else hipLaunchKernelGGL(k_linec_sweep<0>, g, b, 0, s, L, r, z, stop_col, col);
}

static void lc_correct(const LcView &L, double *z, const double *xs, const double *v0, double *part0, double *part1,
                       int grid, const int *stop_col, int col, hipStream_t s, const double *acc = nullptr) {
    const dim3 g(grid), b(NT);
    if (acc) {
        if (L.seg <= 8) hipLaunchKernelGGL(k_linec_correct_acc<7>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col, acc);
        else if (L.seg <= 16) hipLaunchKernelGGL(k_linec_correct_acc<15>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col, acc);
        else if (L.seg <= 25) hipLaunchKernelGGL(k_linec_correct_acc<24>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col, acc);
        else if (L.seg <= 32) hipLaunchKernelGGL(k_linec_correct_acc<31>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col, acc);
        else hipLaunchKernelGGL(k_linec_correct_acc<0>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col, acc);
        return;
    }
    if (L.seg <= 8) hipLaunchKernelGGL(k_linec_correct<7>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col);
    else if (L.seg <= 16) hipLaunchKernelGGL(k_linec_correct<15>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col);
    else if (L.seg <= 25) hipLaunchKernelGGL(k_linec_correct<24>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col);
    else if (L.seg <= 32) hipLaunchKernelGGL(k_linec_correct<31>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col);
    else hipLaunchKernelGGL(k_linec_correct<0>, g, b, 0, s, L, z, xs, v0, part0, part1, stop_col, col);
}

hipError_t launch_linec_setup(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                              const LineC &C, int lev, double *co, unsigned long long *bad, hipStream_t s) {
    if (C.n <= 0) return hipSuccess;
    if (lev < 0 || lev >= C.nlev) return hipErrorInvalidValue;
    const LcView L = lc_view(C, lev);
    const int64_t items = L.nblk * L.nseg * L.jb;
    const dim3 g((unsigned)((items * 64 + NT - 1) / NT)), b(NT);
    const double *cin = lev > 0 ? co : nullptr;
    const int open = C.sp.on && lev == 0 ? 1 : 0;
    if (fp32) hipLaunchKernelGGL(k_linec_setup<float>, g, b, 0, s, L, indptr, indices, (const float *)data, cin, bad + lev, open);
    else hipLaunchKernelGGL(k_linec_setup<double>, g, b, 0, s, L, indptr, indices, (const double *)data, cin, bad + lev, open);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the separators' system: the next level's coefficients (co is free again: the setup launch
    // above has read it, in stream order), or the last level's pivots
    const bool last = lev + 1 == C.nlev;
    hipLaunchKernelGGL(k_linec_reduce, g, b, 0, s, L, last ? nullptr : co, last ? 0 : C.lev[lev + 1].n,
                       last ? C.minv : nullptr, bad + C.nlev);
    return hipGetLastError();
}

hipError_t launch_linec_phase(const LineC &C, int phase, const double *r, double *z, const double *v0, double *part0,
                              double *part1, int grid, const int *stop_col, int col, hipStream_t s, const double *zadd) {
    if (zadd && (phase != 2 || zadd == z)) return hipErrorInvalidValue;
    if (C.n <= 0) {   // a rank without rows: zero partials
        if (phase != 2 || !part0 || grid < 1) return hipSuccess;
        hipError_t e = hipMemsetAsync(part0, 0, (size_t)grid * sizeof(double), s);
        if (e == hipSuccess && part1 && v0) e = hipMemsetAsync(part1, 0, (size_t)grid * sizeof(double), s);
        return e;
    }
    if (C.nlev < 2 || grid < 1) return hipErrorInvalidValue;
    const LcView L0 = lc_view(C, 0);
    if (phase == 0) {
        lc_sweep(L0, r, z, stop_col, col, s);
        return hipGetLastError();
    }
    if (phase == 1) {
        const dim3 b(NT);
        hipLaunchKernelGGL(k_linec_gather, dim3(lc_grid(L0, LC_CAP)), b, 0, s, L0, r, z, C.lev[1].x, stop_col, col);
        for (int lv = 1; lv + 1 < C.nlev; ++lv) {
            const LcView L = lc_view(C, lv);
            double *x = C.lev[lv].x;
            lc_sweep(L, x, x, stop_col, col, s);
            hipLaunchKernelGGL(k_linec_gather, dim3(lc_grid(L, LC_CAP)), b, 0, s, L, x, x, C.lev[lv + 1].x, stop_col, col);
        }
        const LcView LL = lc_view(C, C.nlev - 1);
        hipLaunchKernelGGL(k_linec_serial, dim3(lc_grid(LL, LC_CAP)), b, 0, s, LL, C.lev[C.nlev - 1].x, C.minv, stop_col, col);
        for (int lv = C.nlev - 2; lv >= 1; --lv) {
            const LcView L = lc_view(C, lv);
            lc_correct(L, C.lev[lv].x, C.lev[lv + 1].x, nullptr, nullptr, nullptr, lc_grid(L, LC_CAP), stop_col, col, s);
        }
        return hipGetLastError();
    }
    lc_correct(L0, z, C.lev[1].x, v0, part0, part1, grid, stop_col, col, s, zadd);
    return hipGetLastError();
}

// ---- the rank level's launchers --------------------------------------------------
static bool lc_span_ok(const LineC &C) {
    return C.sp.on && C.n > 0 && C.nlev >= 2 && C.nblk == 1 && C.sp.world >= 1 && C.sp.world <= LINEC_SPAN_MAXW &&
           C.sp.rank >= 0 && C.sp.rank < C.sp.world;
}
static dim3 lc_line_grid(const LineC &C) { return dim3((unsigned)((C.stride + NT - 1) / NT)); }

hipError_t launch_linec_span_rhs(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                                 const LineC &C, int which, double *rhs, hipStream_t s) {
    if (!lc_span_ok(C) || which < 0 || which > 1) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(rhs, 0, (size_t)C.n * sizeof(double), s);
    if (e != hipSuccess) return e;
    const dim3 g = lc_line_grid(C), b(NT);
    if (fp32) hipLaunchKernelGGL(k_linec_span_rhs<float>, g, b, 0, s, C.stride, C.period, indptr, indices, (const float *)data, C.sp.ecol, which, rhs);
    else hipLaunchKernelGGL(k_linec_span_rhs<double>, g, b, 0, s, C.stride, C.period, indptr, indices, (const double *)data, C.sp.ecol, which, rhs);
    return hipGetLastError();
}

hipError_t launch_linec_span_tips(const LineC &C, hipStream_t s) {
    if (!lc_span_ok(C)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_linec_span_tips, lc_line_grid(C), dim3(NT), 0, s, C.stride, C.period, C.n, C.sp.vw, C.sp.tsend);
    return hipGetLastError();
}

hipError_t launch_linec_span_edge(const LineC &C, const double *z, const int *stop_col, int col, hipStream_t s) {
    if (!lc_span_ok(C)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_linec_span_edge, lc_line_grid(C), dim3(NT), 0, s, lc_view(C, 0), z, C.lev[1].x, C.sp.edge, stop_col, col);
    return hipGetLastError();
}

hipError_t launch_linec_span_iface(const LineC &C, unsigned long long *bad, const int *stop_col, int col, hipStream_t s) {
    if (!lc_span_ok(C)) return hipErrorInvalidValue;
    const dim3 g = lc_line_grid(C), b(NT);
    const int W = C.sp.world, me = C.sp.rank;
    const int64_t S = C.stride;
    if (W <= 2) hipLaunchKernelGGL(k_linec_span_iface<2>, g, b, 0, s, S, W, me, C.sp.tips, C.sp.edges, C.sp.xe, bad, stop_col, col);
    else if (W <= 4) hipLaunchKernelGGL(k_linec_span_iface<4>, g, b, 0, s, S, W, me, C.sp.tips, C.sp.edges, C.sp.xe, bad, stop_col, col);
    else if (W <= 8) hipLaunchKernelGGL(k_linec_span_iface<8>, g, b, 0, s, S, W, me, C.sp.tips, C.sp.edges, C.sp.xe, bad, stop_col, col);
    else hipLaunchKernelGGL(k_linec_span_iface<LINEC_SPAN_MAXW>, g, b, 0, s, S, W, me, C.sp.tips, C.sp.edges, C.sp.xe, bad, stop_col, col);
    return hipGetLastError();
}

hipError_t launch_linec_span_correct(const LineC &C, double *z, const double *v0, double *part0, double *part1,
                                     int grid, const int *stop_col, int col, hipStream_t s) {
    if (!lc_span_ok(C) || grid < 1) return hipErrorInvalidValue;
    const LcView L = lc_view(C, 0);
    const dim3 g(grid), b(NT);
    const double *xs = C.lev[1].x, *vw = C.sp.vw, *xe = C.sp.xe;
    if (L.seg <= 8) hipLaunchKernelGGL(k_linec_correct_span<7>, g, b, 0, s, L, z, xs, vw, xe, v0, part0, part1, stop_col, col);
    else if (L.seg <= 16) hipLaunchKernelGGL(k_linec_correct_span<15>, g, b, 0, s, L, z, xs, vw, xe, v0, part0, part1, stop_col, col);
    else if (L.seg <= 25) hipLaunchKernelGGL(k_linec_correct_span<24>, g, b, 0, s, L, z, xs, vw, xe, v0, part0, part1, stop_col, col);
    else if (L.seg <= 32) hipLaunchKernelGGL(k_linec_correct_span<31>, g, b, 0, s, L, z, xs, vw, xe, v0, part0, part1, stop_col, col);
    else hipLaunchKernelGGL(k_linec_correct_span<0>, g, b, 0, s, L, z, xs, vw, xe, v0, part0, part1, stop_col, col);
    return hipGetLastError();
}

}  // namespace vtk
