// vtk_ring.hip — the line-separable and 4D-grid tables' builders, the line path's table SpMV and
// the LDS-ring SpMVs (x-line rings, 4D ring), gfx950.  Built with -ffp-contract=off
// like vtk_kernels.hip: the row sums and the block-Jacobi arithmetic are bit-identical to k_sell.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "vtk_device.hpp"

namespace vtk {

// line-separable values: the table slot of entry (r, c) -- 0 the diagonal D[r], 1 TX[dir][v]
// (line x +- 1 at the row's position v), 2 TV[dir][x] (v +- 1 in the row's line) -- or -1
__device__ __forceinline__ int lsv_slot(int64_t r, int64_t c, int64_t n, int L, int X, int lblk, int64_t &idx) {
    const int64_t x = r / L, v = r % L;
    int64_t dx, vc;
    if (c < n) {
        dx = c / L - x;
        vc = c % L;
        if (lblk < 0) {   // one rank: periodic in x (X >= 3)
            if (dx == X - 1) dx = -1;
            else if (dx == -(X - 1)) dx = 1;
        }
    } else {
        const int64_t kk = c - n, blk = kk / L;
        dx = blk == lblk ? -1 : 1;
        vc = kk % L;
    }
    if (dx == 0) {
        if (vc == v) { idx = r; return 0; }
        if (vc == v - 1 || vc == v + 1) { idx = (int64_t)n + 2 * L + (vc > v ? X : 0) + x; return 2; }
        return -1;
    }
    if ((dx == 1 || dx == -1) && vc == v) { idx = (int64_t)n + (dx > 0 ? L : 0) + v; return 1; }
    return -1;
}

// pass 0: write every entry into its slot (entries sharing a table slot write the same bits when
// the operator is separable; the check pass decides); pass 1: compare every entry bit for bit
__global__ __launch_bounds__(NT) void k_lsv_build(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const double *__restrict__ data, int64_t n, int L, int lblk,
                                                  int xord, double *__restrict__ lsv, int *bad, int pass) {
    const int X = (int)(n / L);
    for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (int64_t)gridDim.x * NT) {
        for (int k = indptr[r]; k < indptr[r + 1]; ++k) {
            int64_t idx;
            if (lsv_slot(r, indices[k], n, L, X, lblk, idx) < 0) {
                atomicOr(bad, 1);
                break;
            }
            if (pass == 0) lsv[idx] = data[k];
            else if (__double_as_longlong(lsv[idx]) != __double_as_longlong(data[k])) atomicOr(bad, 1);
        }
        if (pass == 1) {
            // |= 2: the row is not canonical (its stored columns differ from canon_order's)
            int64_t cxm, cxp;
            const int ord = canon_order(r, n, L, X, lblk, cxm, cxp, xord);
            const int64_t v = r % L;
            int k = indptr[r];
            bool ok = true;
            for (int e = 0; e < 5 && ok; ++e) {
                const int kind = (ord >> (3 * e)) & 7;
                if ((kind == 1 && v == 0) || (kind == 3 && v == L - 1)) continue;
                const int64_t c = kind == 0 ? cxm : (kind == 4 ? cxp : r + kind - 2);
                ok = k < indptr[r + 1] && indices[k] == c;
                ++k;
            }
            if (!ok || k != indptr[r + 1]) atomicOr(bad, 2);
        }
    }
}

hipError_t launch_lsv_build(const int32_t *indptr, const int32_t *indices, const double *data, int64_t n, int L,
                            int lblk, int xord, double *lsv, int *bad, hipStream_t s) {
    if (L <= 0 || n % L != 0 || n / L < 2) return hipErrorInvalidValue;
    int64_t g = (n + NT - 1) / NT;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(k_lsv_build, dim3((unsigned)g), dim3(NT), 0, s, indptr, indices, data, n, L, lblk, xord, lsv, bad, pass);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// 4D grid rows (vtk::Grid4): pass 0 writes every entry's value into its table slot (D[r] for
// the diagonal), pass 1 compares every entry with its slot bit for bit; either pass flags a row
// whose stored columns are not the grid kinds in ascending order.  Rows writing different values
// into one slot leave one of them there, so pass 1 catches every disagreement.
template <typename VT>
__global__ __launch_bounds__(NT) void k_grid4_build(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const VT *__restrict__ data, int64_t n, Grid4 g,
                                                    double *__restrict__ tab, VT *__restrict__ D, int *bad, int pass) {
    for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (int64_t)gridDim.x * NT) {
        const G4Row q = g4_coords(r, g);
        int64_t c[9];
        bool p[9];
        g4_cols(r, q, g, n, c, p);
        int64_t key[9];   // stored-order positions (halo planes: Grid4::xord)
        for (int k = 0; k < 9; ++k) key[k] = k == 0 || k == 8 ? g4_key(c[k], k, n, g) : c[k];
        int ord[9], m = 0;
        for (int k = 0; k < 9; ++k)
            if (p[k]) ord[m++] = k;
        for (int i = 1; i < m; ++i)   // ascending global columns (the stored order of a canonical CSR)
            for (int t = i; t > 0 && key[ord[t]] < key[ord[t - 1]]; --t) {
                const int s = ord[t];
                ord[t] = ord[t - 1];
                ord[t - 1] = s;
            }
        const int k0 = indptr[r];
        bool ok = indptr[r + 1] - k0 == m;
        for (int e = 0; e < m && ok; ++e) {
            const int kind = ord[e];
            if ((int64_t)indices[k0 + e] != c[kind] || (e > 0 && c[ord[e]] == c[ord[e - 1]])) { ok = false; break; }
            const VT dv = data[k0 + e];
            if (kind == 4) {
                if (pass == 0) D[r] = dv;
            } else {
                const int sl = g4_slot(kind, q, g);
                if (pass == 0) tab[sl] = (double)dv;
                else if (__double_as_longlong(tab[sl]) != __double_as_longlong((double)dv)) ok = false;
            }
        }
        if (!ok) atomicOr(bad, 1);
    }
}

hipError_t launch_grid4_build(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                              const Grid4 &g, double *tab, void *D, int *bad, hipStream_t s) {
    const int64_t S4 = (int64_t)g.Ny * g.Nvx * g.Nvy;
    if (g.Ny < 3 || g.Nvx < 2 || g.Nvy < 2 || S4 <= 0 || n % S4 != 0 || n / S4 != g.X || n > INT32_MAX / 2 ||
        (g.lblk < 0 && g.X < 3))
        return hipErrorInvalidValue;
    int64_t gr = (n + NT - 1) / NT;
    if (gr > 4096) gr = 4096;
    if (gr < 1) gr = 1;
    for (int pass = 0; pass < 2; ++pass) {
        if (fp32) hipLaunchKernelGGL(k_grid4_build<float>, dim3((unsigned)gr), dim3(NT), 0, s, indptr, indices,
                                     (const float *)data, n, g, tab, (float *)D, bad, pass);
        else hipLaunchKernelGGL(k_grid4_build<double>, dim3((unsigned)gr), dim3(NT), 0, s, indptr, indices,
                                (const double *)data, n, g, tab, (double *)D, bad, pass);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// y = A x from the line-separable tables and the SELL codes (one wave per 64-row chunk, lane per
// row): k_sell's plain SpMV -- entries in stored order, padding skipped -- reading 12 B of
// matrix per row instead of 44.  lblk < 0: one rank (x couplings periodic); else the halo
// block of the left neighbour line (HALO: the halo columns read from halo[])
// CANON (every row canonical, vtk_csr::lsv_canon): the columns and values from canon_row -- no
// code word or dictionary loaded, the gathers issue with the diagonal
template <bool HALO, bool CANON = false>
__global__ __launch_bounds__(NT) void k_lsv_spmv(const uint32_t *__restrict__ pk, const int32_t *__restrict__ dict,
                                                 const double *__restrict__ lsv, const double *__restrict__ x,
                                                 const double *__restrict__ halo, double *__restrict__ y, int n, int L,
                                                 int lblk, int xord, const int *stop_col, int col) {
    if (stopped(stop_col, col)) return;
    const int lane = threadIdx.x & 63;
    const int X = n / L, nch = (n + 63) >> 6;
    for (int q = (int)(((int64_t)blockIdx.x * NT + threadIdx.x) >> 6); q < nch; q += (int)((int64_t)gridDim.x * NT >> 6)) {
        const int r = 64 * q + lane;
        const bool act = r < n;
        // the row's line and position: the chunk's first row by one division, then the lane
        int xl = (64 * q) / L, v = 64 * q - xl * L + lane;
        while (v >= L) {
            v -= L;
            ++xl;
        }
        const double drow = act ? __builtin_nontemporal_load(lsv + r) : 0.0;
        double s = 0.0;
        if constexpr (CANON) {
            if (act) {
                int c[5];
                double d[5];
                canon_row(lsv, n, L, lblk, xl, v, drow, c, d, xord);
                double xv[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int cc = c[k] >= 0 ? c[k] : r;
                    xv[k] = (HALO && cc >= n) ? halo[cc - n] : x[cc];
                }
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if (c[k] >= 0) s += d[k] * xv[k];
                __builtin_nontemporal_store(s, y + r);
            }
            continue;
        }
        const uint32_t word = act ? __builtin_nontemporal_load(pk + (size_t)q * 64 + lane) : ~0u;
        const int dv = lane < 16 ? dict[(size_t)q * 16 + lane] : 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int code = (int)((word >> (4 * k)) & 15u);
            const int off = __shfl(dv, code, 64);
            if (act && code != PK_CODES) {
                const int c = r + off;
                double val;
                if (off == 0) val = drow;
                else if (off == 1 || off == -1) val = lsv[(size_t)n + 2 * L + (off > 0 ? X : 0) + xl];
                else {
                    const bool up = (HALO && c >= n) ? ((c - n) / L != lblk) : (off == L || (lblk < 0 && off == -(X - 1) * L));
                    val = lsv[(size_t)n + (up ? L : 0) + v];
                }
                const double xv = (HALO && c >= n) ? halo[c - n] : x[c];
                s += val * xv;
            }
        }
        if (act) __builtin_nontemporal_store(s, y + r);
    }
}

// The same SpMV with the x vector staged through LDS (one rank, canonical rows): workgroup (range
// rb, part h) walks the lines of its range in order, loads each line's x rows v0-8 .. v0+LP+7 once
// (coalesced, prefetched one line ahead in registers) into a ring of 4 lines, and forms row v of
// line x from the ring -- x-1 and x+1 at v, x at v-1..v+1 -- with canon_order's straight-line
// sum (the same products added in the same order as k_lsv_spmv<CANON>: bit-identical).  HBM
// reads x once (+2 halo lines per range) instead of gathering it three times from L2/MALL.
__global__ __launch_bounds__(BAND_T) void k_lsv_ring(const double *__restrict__ lsv, const double *__restrict__ x,
                                                     double *__restrict__ y, int n, int L, int H, const int *stop_col,
                                                     int col) {
    __shared__ double ring[4 * BAND_T];
    if (stopped(stop_col, col)) return;
    const int tid = threadIdx.x, X = n / L, LP = L / H;
    const int b = blockIdx.x, R = (int)gridDim.x / H, rb = b / H, h = b % H, v0 = h * LP;
    const int xa = (int)((int64_t)rb * X / R), xb = (int)((int64_t)(rb + 1) * X / R), nl = xb - xa;
    const int v = v0 - 8 + tid;
    const bool inl = v >= 0 && v < L && tid < LP + 16;   // a row of the line (own or v-halo)
    const bool own = tid >= 8 && tid < 8 + LP;
    const double tx0 = own ? lsv[n + v] : 0.0, tx1 = own ? lsv[n + L + v] : 0.0;
    auto line_of = [&](int it) { return it == 0 ? (xa == 0 ? X - 1 : xa - 1) : (it == nl + 1 ? (xb == X ? 0 : xb) : xa - 1 + it); };
    auto slot = [&](int it) { return (it & 3) * BAND_T; };
    // prefetch: x of line_of(it) on the lane's row, D of line it - 1 (computed at iteration it)
    double nxv = inl ? __builtin_nontemporal_load(x + (int64_t)line_of(0) * L + v) : 0.0, nd = 0.0;
    for (int it = 0; it <= nl + 1; ++it) {
        ring[slot(it) + tid] = nxv;
        const double drow = nd;
        if (it <= nl) {
            nxv = inl ? __builtin_nontemporal_load(x + (int64_t)line_of(it + 1) * L + v) : 0.0;
            nd = own && it + 1 >= 2 ? __builtin_nontemporal_load(lsv + (int64_t)(xa + it - 1) * L + v) : 0.0;
        }
        __syncthreads();
        if (it >= 2) {
            const int xl = xa + it - 2;   // line x: ring slots it-2 (x-1), it-1 (x), it (x+1)
            const double tv0 = lsv[n + 2 * L + xl], tv1 = lsv[n + 2 * L + X + xl];
            int64_t cxm, cxp;
            const int ord = __builtin_amdgcn_readfirstlane(canon_order_xv(xl, 0, n, L, X, -1, cxm, cxp));
            const int sx = slot(it - 1);
            const double t0 = tx0 * ring[slot(it - 2) + tid];
            const double t4 = tx1 * ring[slot(it) + tid];
            const double t2 = drow * ring[sx + tid];
            const double t1 = tv0 * ring[sx + tid - (tid > 0 ? 1 : 0)];
            const double t3 = tv1 * ring[sx + tid + (tid < BAND_T - 1 ? 1 : 0)];
            const bool h1 = v > 0, h3 = v < L - 1;
            const double sa = canon_row_sum<false>(ord, t0, t1, t2, t3, t4, h1, h3, 0);
            if (own) st_nt<2>(y + (int64_t)xl * L + v, sa);
        }
    }
}

// 4D grid rows (vtk::Grid4) with x staged through LDS: w = M^-1 A p for the tridiagonal BJ(8)
// (the split DCGS2 step of the 4D operators).  A workgroup of 256 lanes (one row
// each) walks a contiguous range of 256-row groups; an LDS ring of RL doubles holds x over
// [g0 - S3, g0 + 256 + S3) (S3 = Nvx Nvy, the y-line), so the vy, vx and y couplings read LDS, and
// the window slides by one group per step.  Every global operand of a group -- the window's next
// 256 rows, the x -+ 1 plane rows (S4 away: contiguous 256-row blocks), the y-wrap row, m and D --
// is loaded one group ahead into registers, all loads unconditional (clamped rows, the
// halo chosen by address): no exec-masked load, so the wait for a group's operands does not wait
// for the groups behind it.  Coordinates advance by 256 in the mixed radix (no division per row),
// ring slots by 256 modulo RL.  Terms summed in the stored order (as k_sell's grid rows), the BJ
// solve of bj_trim_group: bit-identical to k_sell<EPI_PREC, 8, tri> on the same operator.
// RL: ring length (>= 2 S3 + 512): 4608 (36 KB, four workgroups per CU) when the y-line allows
// (C4: S3 = 2000), else 8192 (64 KB); the tables TX | TY | TVX | TVY (<= G4TAB doubles) in LDS
// too: three workgroups per CU at C4.
// MODE (G4Dots::mode): 0 w = M^-1 A x; 2 DCGS2 step 0 (j = 0: |p|^2, p.w, |w|^2, each lane over
// its own rows); 3 the cycle-start residual r = b - A x, w = M^-1 r, |r|^2, |w|^2 (partials p0,
// p1) -- k_sell<EPI_RESID_PREC>'s operations.  Modes 2-3: one partial per workgroup, lanes ->
// waves -> workgroup in a fixed order.  (Round 5 removed mode 1, the later steps' dots fused in:
// 215.6 vs 201.5 ms per C4 solve)
template <typename VT, bool HALO, int RL, int MODE, int GR>
__global__ __launch_bounds__(GR) __attribute__((amdgpu_waves_per_eu(GR == 512 && RL <= 5120 ? 6 : 1))) void k_g4_ring(Grid4 g, const double *__restrict__ x, const double *__restrict__ halo,
                                                const double *__restrict__ mtri, double *__restrict__ w, int n,
                                                int ngroups_per_wg, int g_lo, int g_hi, G4Dots dd, const int *stop_col,
                                                int col, int fast) {
    constexpr bool RES = MODE == 3;
    // the ring with G4RM-slot mirrors of its ends (slot t < G4RM also at RL + t, t >= RL - G4RM
    // also at t - RL): the +-1 and +-Nvy reads need no wrap
    __shared__ double ring_m[G4RM + RL + G4RM];
    double *const ring = ring_m + G4RM;
    __shared__ double tb[G4TAB];
    __shared__ double red3[3][MODE >= 2 ? GR / 64 : 1];
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;   // MODE 2 / 3: the lane's sums over its rows
    if (stopped(stop_col, col)) return;
    const int tid = threadIdx.x, lane = tid & 63, ii = lane & 7;
    const int Nvy = g.Nvy, Nvx = g.Nvx, Ny = g.Ny;
    const int S2 = Nvy, S3 = Nvx * Nvy, S4 = Ny * S3;
    const int gb = g_lo + blockIdx.x * ngroups_per_wg, ge = min(g_hi, gb + ngroups_per_wg);
    const int pslot = dd.part_off + blockIdx.x;   // this workgroup's partial slot
    if (gb >= ge) {   // (no work: zero partials, so that the slots' consumers need no count)
        if (MODE >= 1 && threadIdx.x < DC_NQ) {
            const int q = threadIdx.x;
            if (MODE == 3) { if (q == 0) dd.p0[pslot] = 0.0; if (q == 1) dd.p1[pslot] = 0.0; }
            else if (q >= 2 * DC_MAXJ) dd.part[(size_t)q * GMAX + pslot] = 0.0;
        }
        return;
    }
    const int oy = 2 * Nvx, ovx = oy + 2 * Nvy, ovy = ovx + 2 * g.X;
    const int lb = g.lblk;
    // the value tables in LDS (a table load in the row loop would be a global load issued after
    // the queue's prefetch: waiting for it would wait for the whole queue)
    for (int i = tid; i < ovy + 2 * Ny; i += GR) tb[i] = g.tab[i];
    // the window's initial rows [gb GR - S3, gb GR + GR + S3), clamped to [0, n)
    for (int r = gb * GR - S3 + tid; r < gb * GR + GR + S3; r += GR)
        if (r >= 0 && r < n) {
            const int t = r % RL;
            const double v = x[r];
            ring[t] = v;
            if (t < G4RM) ring[RL + t] = v;
            if (t >= RL - G4RM) ring[t - RL] = v;
        }
    // GR in the mixed radix (Nvy, Nvx, Ny, X)
    const int a0 = GR % Nvy, q0 = GR / Nvy, a1 = q0 % Nvx, q1 = q0 / Nvx, a2 = q1 % Ny, a3 = q1 / Ny;
    struct Co {
        int jvy, jvx, iy, ix;
    };
    auto adv = [&](Co &c) {
        c.jvy += a0;
        int cy = c.jvy >= Nvy;
        c.jvy -= cy ? Nvy : 0;
        c.jvx += a1 + cy;
        cy = c.jvx >= Nvx;
        c.jvx -= cy ? Nvx : 0;
        c.iy += a2 + cy;
        cy = c.iy >= Ny;
        c.iy -= cy ? Ny : 0;
        c.ix += a3 + cy;
    };
    // the x -+ 1 plane columns of row rc (one rank: periodic inside the slab; else halo planes)
    auto xcols = [&](int rc, int &cm, int &cp) {
        if (!HALO) {
            cm = rc >= S4 ? rc - S4 : rc + (n - S4);
            cp = rc < n - S4 ? rc + S4 : rc - (n - S4);
        } else {
            cm = rc >= S4 ? rc - S4 : n + lb * S4 + rc;
            cp = rc < n - S4 ? rc + S4 : (1 - lb) * S4 + rc + S4;
        }
    };
    // element i of a kernel-argument array through a 32-bit byte offset (i < 2^28): the load
    // takes the array base in SGPRs and the offset in one VGPR (no 64-bit address per lane)
    auto at = [](const auto *base, int i) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(base)>>;
        return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (uint32_t)i * (uint32_t)sizeof(T));
    };
    auto atn = [](const auto *base, int i) {   // (non-temporal: the streamed operands)
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(base)>>;
        return __builtin_nontemporal_load(
            reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (uint32_t)i * (uint32_t)sizeof(T)));
    };
    auto xat = [&](int c) { return HALO ? *(c >= n ? halo + (c - n) : x + c) : at(x, c); };
    struct Ld {
        double xn, xm, xp, xw, m, d, b;
        Co c;
    };
    Co lead;
    {
        const int r = gb * GR + tid;
        lead.jvy = r % Nvy;
        const int t1 = r / Nvy;
        lead.jvx = t1 % Nvx;
        const int t2 = t1 / Nvx;
        lead.iy = t2 % Ny;
        lead.ix = t2 / Ny;
    }
    auto load = [&](int gl, Ld &o) {
        const int r = gl * GR + tid;
        const int rc = min(r, n - 1);
        o.xn = at(x, min(r + GR + S3, n - 1));
        int cm, cp;
        xcols(rc, cm, cp);
        o.xm = xat(cm);
        o.xp = xat(cp);
        const int cw = lead.iy == 0 ? rc + (Ny - 1) * S3 : (lead.iy == Ny - 1 ? rc - (Ny - 1) * S3 : rc);
        o.xw = at(x, min(max(cw, 0), n - 1));
        o.m = atn(mtri, rc);
        o.d = (double)atn(static_cast<const VT *>(g.D), rc);
        o.b = RES ? atn(dd.b, rc) : 0.0;
        o.c = lead;
        adv(lead);
    };
    Ld nx;
    load(gb, nx);
    int sb = (gb * GR + tid) % RL;   // ring slot of the lane's row
    auto slotp = [&](int off) {   // sb + off, 0 <= off < RL
        const int t = sb + off;
        return t >= RL ? t - RL : t;
    };
    auto slotm = [&](int off) {   // sb - off, 0 <= off < RL
        const int t = sb - off;
        return t < 0 ? t + RL : t;
    };
    __syncthreads();
    for (int gi = gb; gi < ge; ++gi) {
        const Ld cu = nx;
        // the next group's operands; across ranks not past the range's last group: the interior
        // launch runs while the comm stream writes the halo planes, which a group beyond its
        // range would read (the value was never used, the read still raced the write)
        load(HALO ? min(gi + 1, ge - 1) : gi + 1, nx);
        const int r = gi * GR + tid;
        const bool act = r < n;
        const int rc = act ? r : n - 1;
        const int jvy = cu.c.jvy, jvx = cu.c.jvx, iy = cu.c.iy, ix = cu.c.ix;
        const bool pvm = jvx > 0, pvp = jvx < Nvx - 1, pym = jvy > 0, pyp = jvy < Nvy - 1;
        const double xvm = ring[sb - S2], xvp = ring[sb + S2];   // (mirrored ends)
        const double xwm = ring[sb - 1], xwp = ring[sb + 1];
        const double x0 = ring[sb];
        const int jx = min(jvx, Nvx - 1), jy = min(jvy, Nvy - 1), kx = min(ix, g.X - 1), ky = min(iy, Ny - 1);
        const double t0 = tb[jx] * cu.xm, t8 = tb[Nvx + jx] * cu.xp;
        const double d2 = tb[ovx + kx], d6 = tb[ovx + g.X + kx], d3 = tb[ovy + ky], d5 = tb[ovy + Ny + ky];
        const double t2v = d2 * xvm, t6 = d6 * xvp, t3 = d3 * xwm, t5 = d5 * xwp, t4 = cu.d * x0;
        double s = 0.0;
        // a wave whose rows all sit inside the slab's x range and the y range (no periodic wrap, no
        // halo plane): the stored order is x-1, y-1, vx-1, vy-1, diag, vy+1, vx+1, y+1, x+1 -- the
        // general form's select chains below reduce to it term for term (the same adds in the same
        // order), without the column keys (C4: the waves off a y-line's or a slab's edge, ~95 %)
        const bool inner = act && rc >= S4 && rc < n - S4 && iy > 0 && iy < Ny - 1;
        if (fast && __builtin_amdgcn_ballot_w64(!inner) == 0) {
            const double t1y = tb[oy + jy] * ring[slotm(S3)], t7 = tb[oy + Nvy + jy] * ring[slotp(S3)];
            s = s + t0;
            s = s + t1y;
            s = pvm ? s + t2v : s;
            s = pym ? s + t3 : s;
            s = s + t4;
            s = pyp ? s + t5 : s;
            s = pvp ? s + t6 : s;
            s = s + t7;
            s = s + t8;
        } else {
            // in-plane neighbours from the ring (y wraps from the queue)
            const int cym = iy == 0 ? rc + (Ny - 1) * S3 : rc - S3;
            const int cyp = iy == Ny - 1 ? rc - (Ny - 1) * S3 : rc + S3;
            const double xym = iy == 0 ? cu.xw : ring[slotm(S3)];
            const double xyp = iy == Ny - 1 ? cu.xw : ring[slotp(S3)];
            const double t1y = tb[oy + jy] * xym, t7 = tb[oy + Nvy + jy] * xyp;
            int cm, cp;
            xcols(rc, cm, cp);
            const int64_t km = g4_key(cm, 0, n, g), kp = g4_key(cp, 8, n, g);   // stored-order positions
            auto add2 = [&](bool pa, int64_t ca, double ta, bool pb, int64_t cb, double tb2) {
                const bool sw = pa && pb && cb < ca;
                const double u1 = sw ? tb2 : ta, u2 = sw ? ta : tb2;
                const bool p1 = sw ? pb : pa, p2 = sw ? pa : pb;
                s = p1 ? s + u1 : s;
                s = p2 ? s + u2 : s;
            };
            add2(km < rc, km, t0, kp < rc, kp, t8);
            add2(cym < rc, cym, t1y, cyp < rc, cyp, t7);
            s = pvm ? s + t2v : s;
            s = pym ? s + t3 : s;
            s = s + t4;
            s = pyp ? s + t5 : s;
            s = pvp ? s + t6 : s;
            add2(cym > rc, cym, t1y, cyp > rc, cyp, t7);
            add2(km > rc, km, t0, kp > rc, kp, t8);
        }
        const double sub = (pym && ii > 0) ? 0.0 + d3 : 0.0, sup = (pyp && ii < 7) ? 0.0 + d5 : 0.0;
        // BJ, store and sums; ALL: every lane of the wave holds a row (all but the last group's
        // waves), so no lane needs the inactive-lane selects
        auto epi = [&](const bool all) {
            const bool on = all || act;
            double sv = s;
            if constexpr (RES) {   // r = b - A x (iterative.py:816)
                sv = on ? cu.b - s : 0.0;
                e0 += sv * sv;
            }
            const double z = bj_trim_group<8>(on ? sv : 0.0, lane, on ? sub : 0.0, on ? sup : 0.0, on ? cu.m : 1.0);
            if (on) st_nt<2>(reinterpret_cast<double *>(reinterpret_cast<char *>(w) + (uint32_t)r * 8u), z);
            if constexpr (RES) {
                if (on) e1 += z * z;
            } else if constexpr (MODE == 2) {
                if (on) {
                    e0 += x0 * x0;
                    e1 += x0 * z;
                    e2 += z * z;
                }
            }
        };
        if (__builtin_amdgcn_ballot_w64(!act) == 0) epi(true);
        else epi(false);
        // slide the window: the rows of group gi + 1's upper edge (their slots held rows the
        // remaining groups no longer read; the ring is > 2 S3 + 512 long)
        if (r + GR + S3 < n) {
            const int t = slotp(GR + S3);
            ring[t] = cu.xn;
            if (t < G4RM) ring[RL + t] = cu.xn;
            if (t >= RL - G4RM) ring[t - RL] = cu.xn;
        }
        sb = slotp(GR);
        __syncthreads();
    }
    if constexpr (MODE >= 2) {
        const int wid = tid >> 6;
        const double t0 = wave_sum(e0), t1 = wave_sum(e1), t2 = wave_sum(e2);
        if (lane == 0) {
            red3[0][wid] = t0;
            red3[1][wid] = t1;
            red3[2][wid] = t2;
        }
        __syncthreads();
        if (tid < 3) {
            double sum = 0.0;
#pragma unroll
            for (int wv = 0; wv < GR / 64; ++wv) sum += red3[tid][wv];
            if constexpr (MODE == 2) dd.part[(size_t)(2 * DC_MAXJ + tid) * GMAX + pslot] = sum;
            else if (tid == 0) dd.p0[pslot] = sum;
            else if (tid == 1) dd.p1[pslot] = sum;
        }
    }
}

hipError_t launch_g4_ring(const Grid4 &g, const double *x, const double *halo, const double *mtri, double *w, int64_t n,
                          int fp32, int wgs, int gr, const G4Dots *dots, int *grid_out, const int *stop_col,
                          int col, hipStream_t s, int g_lo, int g_hi, int per_in, int fast) {
    // gr: rows per group = lanes per workgroup (256 or 512)
    const int mode = dots ? dots->mode : 0;
    const int G = g4_ring_group(gr);
    const int64_t S3 = (int64_t)g.Nvx * g.Nvy, S4 = S3 * g.Ny;
    if (!g.tab || !g.D || !g4_ring_fits(g, n, gr) || S4 <= 0 || n % S4 || (halo == nullptr) != (g.lblk < 0))
        return hipErrorInvalidValue;
    // the ring: the window 2 S3 + G plus the next group's rows
    const bool small = 2 * S3 + 2 * G <= (G == 256 ? 4608 : 5120);
    const int64_t ng = (n + G - 1) / G;
    int64_t per = g4_ring_per(ng, S4, G, wgs);
    // the fused reductions write one partial per workgroup: at most GMAX workgroups
    if (mode) per = std::max<int64_t>(per, (ng + GMAX - 1) / GMAX);
    // a group range [g_lo, g_hi) of the launch (the interior / boundary planes of a rank's slab
    // around the halo exchange), groups per workgroup per_in > 0 as the caller planned them
    if (g_hi < 0) g_hi = (int)ng;
    if (per_in > 0) per = per_in;
    if (g_lo < 0 || g_lo > g_hi || g_hi > ng) return hipErrorInvalidValue;
    const int64_t span = std::max<int64_t>(1, g_hi - g_lo);
    const dim3 grid((unsigned)((span + per - 1) / per)), blk(G);
    if (mode && (dots->part_off < 0 || dots->part_off + (int64_t)grid.x > GMAX)) return hipErrorInvalidValue;
    if (mode == 1 || mode < 0 || mode > 3 || (mode == 2 && !dots->part) ||
        (mode == 3 && (!dots->b || !dots->p0 || !dots->p1)))
        return hipErrorInvalidValue;
    if (grid_out) *grid_out = (int)grid.x;
    const G4Dots dd = dots ? *dots : G4Dots{};
#define VTK_G4R(VT_, H_, RL_, M_, GR_) \
    hipLaunchKernelGGL((k_g4_ring<VT_, H_, RL_, M_, GR_>), grid, blk, 0, s, g, x, halo, mtri, w, (int)n, (int)per, g_lo, \
                       g_hi, dd, stop_col, col, fast)
#define VTK_G4R_M(VT_, H_, RL_, GR_) \
    do { \
        if (mode == 2) VTK_G4R(VT_, H_, RL_, 2, GR_); \
        else if (mode == 3) VTK_G4R(VT_, H_, RL_, 3, GR_); \
        else VTK_G4R(VT_, H_, RL_, 0, GR_); \
    } while (0)
#define VTK_G4R_PD(VT_, H_) \
    do { \
        if (G == 512) { if (small) VTK_G4R_M(VT_, H_, 5120, 512); else VTK_G4R_M(VT_, H_, 8192, 512); } \
        else if (small) VTK_G4R_M(VT_, H_, 4608, 256); \
        else VTK_G4R_M(VT_, H_, 8192, 256); \
    } while (0)
    if (fp32) {
        if (halo) VTK_G4R_PD(float, true);
        else VTK_G4R_PD(float, false);
    } else {
        if (halo) VTK_G4R_PD(double, true);
        else VTK_G4R_PD(double, false);
    }
#undef VTK_G4R_PD
#undef VTK_G4R_M
#undef VTK_G4R
    return hipGetLastError();
}

// k_lsv_ring with the solver's epilogues (one rank, canonical rows): the row sum
// exactly as k_lsv_ring / k_sell's canonical rows, then
//   EPI_RESID       r = b - A x -> y, |r|^2                         (cycle start, line path)
//   EPI_RESID_PREC  r = b - A x, z = M^-1 r -> y, |r|^2, |z|^2      (cycle start, BJ(8))
//   EPI_PREC_DC     z = M^-1 A x -> y, |x|^2, x.z, |z|^2            (DCGS2 step 0, BJ(8))
// with M^-1 the tridiagonal BJ(8) of bj_trim_group (the same operations as k_sell's TRIM
// epilogue).  The reductions: per lane over its rows in line order, then wave_sum, then the
// waves in order -- one partial per workgroup (PREC_DC: launch_dc_dots' layout).
//   EPI_PREC_DC_ND  EPI_PREC_DC as z = x + M^-1 (C x), no read of D (the band step's BAND_ND):
//                   step 0 of a band cycle forms its w by the same operator expression as the
//                   band steps after it.  The residual epilogues keep D: they need r = b - A x
// halo (distributed, vtk_csr::band_ghost): the two neighbour lines (blocks lblk = left and
// 1 - lblk = right of L doubles, after halo_exchange), xord their place in the stored order
struct LsvEpiK {
    const double *lsv, *x, *b, *mtri;
    double *y, *p0, *p1, *dcpart;
    int n, L, H;
    const int *stop_col;
    int col;
    const double *halo;
    int lblk, xord;
};
template <int EPI_>
__global__ __launch_bounds__(BAND_T) void k_lsv_ring_epi(LsvEpiK a) {
    constexpr bool ND = EPI_ == EPI_PREC_DC_ND;
    constexpr int EPI = ND ? (int)EPI_PREC_DC : EPI_;
    __shared__ double ring[4 * BAND_T];
    __shared__ double red[3][BAND_T / 64];
    if (stopped(a.stop_col, a.col)) return;
    const double *__restrict__ lsv = a.lsv;
    const double *__restrict__ x = a.x;
    const int n = a.n, L = a.L, H = a.H;
    const int tid = threadIdx.x, lane = tid & 63, ii = lane & 7, X = n / L, LP = L / H;
    const int b = blockIdx.x, R = (int)gridDim.x / H, rb = b / H, h = b % H, v0 = h * LP;
    const int xa = (int)((int64_t)rb * X / R), xb = (int)((int64_t)(rb + 1) * X / R), nl = xb - xa;
    const int v = v0 - 8 + tid;
    const bool inl = v >= 0 && v < L && tid < LP + 16;
    const bool own = tid >= 8 && tid < 8 + LP;
    const double tx0 = own ? lsv[n + v] : 0.0, tx1 = own ? lsv[n + L + v] : 0.0;
    auto line_of = [&](int it) { return it == 0 ? (xa == 0 ? X - 1 : xa - 1) : (it == nl + 1 ? (xb == X ? 0 : xb) : xa - 1 + it); };
    // the rows of iteration it's line: x, or a neighbour rank's line (the slab's x-halo) in halo
    const double *hal = a.halo;
    auto line_ptr = [&](int it) -> const double * {
        if (hal && it == 0 && xa == 0) return hal + (int64_t)a.lblk * L;
        if (hal && it == nl + 1 && xb == X) return hal + (int64_t)(1 - a.lblk) * L;
        return x + (int64_t)line_of(it) * L;
    };
    auto slot = [&](int it) { return (it & 3) * BAND_T; };
    constexpr bool BJ = EPI == EPI_RESID_PREC || EPI == EPI_PREC_DC;
    constexpr bool HB = EPI == EPI_RESID || EPI == EPI_RESID_PREC;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    // prefetch: x of line_of(it), and D (m, b) of line it - 1 (computed at iteration it)
    double nxv = inl ? __builtin_nontemporal_load(line_ptr(0) + v) : 0.0, nd = 0.0, nm = 1.0, nb = 0.0;
    for (int it = 0; it <= nl + 1; ++it) {
        ring[slot(it) + tid] = nxv;
        const double drow = nd, mrow = nm, brow = nb;
        if (it <= nl) {
            nxv = inl ? __builtin_nontemporal_load(line_ptr(it + 1) + v) : 0.0;
            if (own && it + 1 >= 2) {
                const int64_t rr = (int64_t)(xa + it - 1) * L + v;
                if constexpr (!ND) nd = __builtin_nontemporal_load(lsv + rr);
                if constexpr (BJ) nm = __builtin_nontemporal_load(a.mtri + rr);
                if constexpr (HB) nb = __builtin_nontemporal_load(a.b + rr);
            }
        }
        __syncthreads();
        if (it >= 2) {
            const int xl = xa + it - 2;
            const double tv0 = lsv[n + 2 * L + xl], tv1 = lsv[n + 2 * L + X + xl];
            int64_t cxm, cxp;
            const int ord = __builtin_amdgcn_readfirstlane(canon_order_xv(xl, 0, n, L, X, hal ? a.lblk : -1, cxm, cxp, a.xord));
            const int sx = slot(it - 1);
            const double t0 = tx0 * ring[slot(it - 2) + tid];
            const double t4 = tx1 * ring[slot(it) + tid];
            const double xr = ring[sx + tid];
            const double t2 = drow * xr;
            const double t1 = tv0 * ring[sx + tid - (tid > 0 ? 1 : 0)];
            const double t3 = tv1 * ring[sx + tid + (tid < BAND_T - 1 ? 1 : 0)];
            const bool h1 = v > 0, h3 = v < L - 1;
            const double sa = canon_row_sum<ND>(ord, t0, t1, t2, t3, t4, h1, h3, ii);
            const int64_t row = (int64_t)xl * L + v;
            double out = sa;
            if constexpr (HB) {
                out = own ? brow - sa : 0.0;   // r = b - A x
                acc0 += out * out;
            }
            if constexpr (BJ) {
                const double sub = (own && h1 && ii > 0) ? 0.0 + tv0 : 0.0;
                const double sup = (own && h3 && ii < 7) ? 0.0 + tv1 : 0.0;
                double z = bj_trim_group<8>(own ? out : 0.0, lane, sub, sup, own ? mrow : 1.0);
                if constexpr (ND) z = xr + z;   // x + M^-1 (C x)
                if constexpr (EPI == EPI_RESID_PREC) {
                    if (own) acc1 += z * z;
                } else {
                    if (own) {
                        acc0 += xr * xr;
                        acc1 += xr * z;
                        acc2 += z * z;
                    }
                }
                out = z;
            }
            if (own) st_nt<2>(a.y + row, out);
        }
    }
    const int wid = tid >> 6;
    const double t0 = wave_sum(acc0), t1 = wave_sum(acc1), t2 = wave_sum(acc2);
    if (lane == 0) {
        red[0][wid] = t0;
        red[1][wid] = t1;
        red[2][wid] = t2;
    }
    __syncthreads();
    if (tid < 3) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < BAND_T / 64; ++w) sum += red[tid][w];
        if constexpr (EPI == EPI_PREC_DC) a.dcpart[(size_t)(2 * DC_MAXJ + tid) * GMAX + b] = sum;
        else if (tid == 0) a.p0[b] = sum;
        else if (tid == 1 && EPI == EPI_RESID_PREC) a.p1[b] = sum;
    }
}

hipError_t launch_lsv_ring_epi(int epi, const double *lsv, const double *x, const double *b, const double *mtri,
                               double *y, double *p0, double *p1, double *dcpart, int64_t n, int L, int ring_wgs,
                               const int *stop_col, int col, int *grid_out, hipStream_t s, const double *halo, int lblk,
                               int xord) {
    const int H = band_parts(L);
    const int64_t X = L > 0 ? n / L : 0;
    if (n <= 0 || n > INT32_MAX / 2 || L <= 0 || n % L != 0 || H < 1 || X < (halo ? 2 : 3) || ring_wgs < 1 ||
        (halo && (lblk < 0 || lblk > 1)))
        return hipErrorInvalidValue;
    const bool dc = epi == EPI_PREC_DC || epi == EPI_PREC_DC_ND;
    const bool bj = epi == EPI_RESID_PREC || dc;
    if ((bj && !mtri) || ((epi == EPI_RESID || epi == EPI_RESID_PREC) && (!b || !p0)) ||
        (epi == EPI_RESID_PREC && !p1) || (dc && !dcpart) || L % 8 != 0)
        return hipErrorInvalidValue;
    // one partial per workgroup: at most GMAX
    const int64_t R = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ring_wgs / H, X / 2), GMAX / H));
    LsvEpiK a{lsv, x, b, mtri, y, p0, p1, dcpart, (int)n, L, H, stop_col, col, halo, halo ? lblk : -1, halo ? xord : 0};
    const dim3 g((unsigned)(R * H)), blk(BAND_T);
    if (grid_out) *grid_out = (int)g.x;
    switch (epi) {
        case EPI_RESID: hipLaunchKernelGGL(k_lsv_ring_epi<EPI_RESID>, g, blk, 0, s, a); break;
        case EPI_RESID_PREC: hipLaunchKernelGGL(k_lsv_ring_epi<EPI_RESID_PREC>, g, blk, 0, s, a); break;
        case EPI_PREC_DC: hipLaunchKernelGGL(k_lsv_ring_epi<EPI_PREC_DC>, g, blk, 0, s, a); break;
        case EPI_PREC_DC_ND: hipLaunchKernelGGL(k_lsv_ring_epi<EPI_PREC_DC_ND>, g, blk, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_lsv_spmv(const uint32_t *pk, const int32_t *dict, const double *lsv, const double *x,
                           const double *halo, double *y, int64_t n, int L, int lblk, const int *stop_col, int col,
                           hipStream_t s, int canon, int grid_cap, int ring_wgs, int xord) {
    if (n <= 0 || n > INT32_MAX / 2 || L <= 0 || n % L != 0 || (halo && lblk < 0)) return hipErrorInvalidValue;
    if (ring_wgs > 0 && canon && !halo) {   // the LDS-staged form (one rank, canonical rows)
        const int H = band_parts(L);
        const int64_t X = n / L;
        if (H >= 1 && X >= 3) {
            const int64_t R = std::max<int64_t>(1, std::min<int64_t>(ring_wgs / H, X / 2));
            hipLaunchKernelGGL(k_lsv_ring, dim3((unsigned)(R * H)), dim3(BAND_T), 0, s, lsv, x, y, (int)n, L, H, stop_col, col);
            return hipGetLastError();
        }
    }
    const int64_t nch = (n + 63) / 64;
    // grid_cap: 8192 workgroups by default (vtk::Tuning::lsv_spmv_cap; C3 line solve, in-process
    // A/B: 8.69 ms vs 8.73 at 2048 and 8.85 with one chunk per wave; an XCD swizzle of the chunks
    // 8.81 vs 8.70)
    const int64_t cap = grid_cap > 0 ? grid_cap : 8192;
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>((nch + 3) / 4, cap));
    if (canon && halo) hipLaunchKernelGGL((k_lsv_spmv<true, true>), dim3((unsigned)g), dim3(NT), 0, s, pk, dict, lsv, x, halo, y, (int)n, L, lblk, xord, stop_col, col);
    else if (canon) hipLaunchKernelGGL((k_lsv_spmv<false, true>), dim3((unsigned)g), dim3(NT), 0, s, pk, dict, lsv, x, halo, y, (int)n, L, lblk, xord, stop_col, col);
    else if (halo) hipLaunchKernelGGL(k_lsv_spmv<true>, dim3((unsigned)g), dim3(NT), 0, s, pk, dict, lsv, x, halo, y, (int)n, L, lblk, xord, stop_col, col);
    else hipLaunchKernelGGL(k_lsv_spmv<false>, dim3((unsigned)g), dim3(NT), 0, s, pk, dict, lsv, x, halo, y, (int)n, L, lblk, xord, stop_col, col);
    return hipGetLastError();
}

}  // namespace vtk
