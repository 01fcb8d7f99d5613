// vtk_band.hip — the line-band DCGS2 step and its ghost-line exchange and
// structure checks, gfx950.  Built with -ffp-contract=off like vtk_kernels.hip: the update,
// SpMV and block-Jacobi arithmetic is bit-identical to k_dc_update / k_sell.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "vtk_device.hpp"

namespace vtk {

// ------------------------------------------------------------------------------------------
// Line-band DCGS2 step.  For an operator whose rows form x-lines of L rows
// (row = x L + v) with every column in lines x-1, x, x+1 (periodic in x) at v-1..v+1 -- the 2D
// Vlasov operators, L = Nv -- the update pass of step j and the fused SpMV + BJ + dots of step
// j+1 run as ONE sweep.  Workgroup (range r, part h) owns rows v0 <= v < v0 + LP (LP = L / H)
// of the lines [xa, xb) of range r and walks them in order; at line x it
//   1. updates line x+1 on its rows plus one v-halo row on each side: recomputes p_j exactly as
//      step j-1 formed it, p_j = (w_{j-1} - sum_k e'_k V_k) q' (the previous step's scalars e',
//      q' in DcCoef::e_prev / q_prev; p_0 = v_0), then v_j and p_{j+1} as k_dc_update, and puts
//      p_{j+1}(x+1) into an LDS ring of 4 lines,
//   2. computes w(x) = M^-1 A p_{j+1} on its rows of line x from the ring (the SELL entries in
//      stored order and the tridiagonal BJ solve exactly as k_sell: w is bit-identical),
//   3. accumulates step j+1's dots s = V_{j+1}^T p_{j+1}, z = V_{j+1}^T w, |p|^2, p.w, |w|^2
//      from LDS: the line's basis rows were staged there by step 1 one line earlier.
// The basis is read from HBM once per step instead of twice (update pass + dots), p_{j+1} is
// neither stored (except by the last band step, whose successor is k_dc_update) nor re-read
// for the SpMV gathers, and one launch replaces two.  Rows another workgroup owns are
// recomputed from that row's own V_k, w_{j-1}, w_j: the x-halo lines xa-1 and xb and the v-halo
// rows v0-1, v0+LP -- no per-step boundary copies between workgroups.  w cycles through three
// buffers (w_{j-1}, w_j read, w_{j+1} written).  7 waves; lane tid <-> row v = v0 - 16 + tid
// (8-row BJ blocks stay lane-aligned); ~79 KB LDS: two workgroups per CU, whose update / SpMV /
// dots phases overlap.
// Below: the walk, then the phases in the order of a line iteration, then the kernel, which reads
// as the list above.  The variant bits: BandOpt, vtk_internal.hpp.
// ------------------------------------------------------------------------------------------

// geometry: half lines (LP <= BAND_LP = 400 rows, 7 waves, ~79 KB LDS, two workgroups per CU).
// Quarter lines with the staged basis double-buffered and every step's next line prefetched
// (4 waves, 2-4 workgroups per CU by LDS) measured 2-10 % slower per step (round 5).
#define VTK_BAND_DOTS_UNROLL 2   // (a #pragma unroll literal) the dots' 64-row passes issued together
constexpr int BAND_XUP_XB = 4;     // the cycle's x update inlined into k_band_step, basis loads in batches of
                                   // this many (C3 x update 648-653 -> 641-643 us)
constexpr int BAND_PF = 12;        // j <= this: next line's update operands prefetched across SpMV + dots
                                   // (round 3: 10: 567-570 us; 8: 570; 12: 567; 18: 624, spills; with
                                   // the fused multiply-adds j <= 12 fits 124 VGPRs)
constexpr int BAND_W = BAND_T / 64;   // waves per workgroup
template <int J> constexpr int band_items() { return (J + 2 + BAND_W - 1) / BAND_W; }   // dot items per wave

// VMODE 1 (LSV): the matrix values from the line-separable tables (vtk_csr::d_lsv: the diagonal
// per row, x +- 1 couplings per position v -- held in registers for the lane's v --, v +- 1
// couplings per line) instead of the SELL copy's 5 values per row; VMODE 2 (also canonical
// rows, vtk_csr::lsv_canon): the entries' kinds and order from canon_order instead of the SELL
// codes and dictionary.  The same values in the same order either way.
// The update's sums and the dots are fused multiply-adds (one rounding per term, half the f64
// VALU instructions of the separate multiply and add; C3 solve -1 %, round 5); p_j's recompute
// (here and in the x update's) is the same fused chain, so step j forms p_j exactly as step j-1
// did.  (k_dc_update keeps the unfused operations of the oracle's sequence.)
__device__ __forceinline__ double band_msub(double acc, double a, double b) { return __builtin_fma(-a, b, acc); }
__device__ __forceinline__ double band_madd(double acc, double a, double b) { return __builtin_fma(a, b, acc); }
template <int OPT> constexpr int band_wpe() { return (OPT & BAND_WPC3) ? 6 : 4; }   // waves per SIMD
// BAND_XCDP: logical block (range, part) = (8 (b / 16) + b mod 8, (b / 8) mod 2): blockIdx b and b + 8 share
// an XCD's L2.  The logical index also names the workgroup's partial slot, so the dots' sums keep their bits.
__device__ __forceinline__ int band_block(int opt, int H) {
    const int b = blockIdx.x;
    if (!(opt & BAND_XCDP) || H != 2 || (gridDim.x & 15) != 0) return b;
    return (((b >> 4) << 3) + (b & 7)) * 2 + ((b >> 3) & 1);
}
// BAND_L2PF: bare s_barriers after lgkmcnt(0) -- __syncthreads' release fence would wait for the DMA (vmcnt(0))
// at every barrier.  Only LDS is shared inside the kernel, so lgkmcnt(0) + s_barrier orders all the barrier has to.
template <int OPT> __device__ __forceinline__ void band_sync() {
    if constexpr (OPT & BAND_L2PF) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}
// lane tid <-> row v0 - BAND_OFF + tid: 16 rows (128 B) ahead of the part's first row, so that a
// wave's 64 rows are one aligned 512-B run of every row vector (four cache lines; with 8, the BJ
// blocks' minimum, five: round 6), the 8-row BJ blocks lane-aligned, the v-halo rows at tid
// BAND_OFF - 1 and BAND_OFF + LP (LP + 2 BAND_OFF <= BAND_T)
constexpr int BAND_OFF = 16;
static_assert(BAND_LP + 2 * BAND_OFF <= BAND_T && BAND_OFF % 8 == 0, "band geometry");

// the lane's place in its workgroup's part h of a line
struct BandLane {
    int tid, lane, wv, ii;
    int L, X, LP, v0, v;
    bool own, upd;   // a row of the part; ... or one of its two v-halo rows (updated, not owned)
    __device__ __forceinline__ BandLane(const BandK &a, int h)
        : tid(threadIdx.x), lane(tid & 63), wv(tid >> 6), ii(lane & 7), L(a.L), X(a.X), LP(L / a.H_parts), v0(h * LP),
          v(v0 - BAND_OFF + tid), own(tid >= BAND_OFF && tid < BAND_OFF + LP),
          upd(tid >= BAND_OFF - 1 && tid <= LP + BAND_OFF && v >= 0 && v < L) {}
};

// ---- the walk ------------------------------------------------------------------------------
// Iteration it = 0 .. nl + 1 of line range [xa, xb) updates one line and, from it = 2 on, runs
// the SpMV and dots of the line updated one iteration before, whose x-neighbours are both in
// the ring then.  A forward walk updates y = xa - 1 + it and works on y - 1; a reversed one
// (BAND_ALT: odd ranges; BAND_SERP: odd steps on top of it -- both workgroups at a range boundary
// flip together, so ALT's pairing holds) updates y = xb - it and works on y + 1.  The first and
// last iterations update the x-halo lines (recomputed, nothing stored), which on a rank's outermost
// ranges are a neighbour rank's lines in the ghost buffer.  Only this struct knows the direction
// and the ghost buffer's layout.
struct BandLine {
    int y, kind;   // the line (mod X); 0 owned, 1 / 2 the left / right x-halo line
    int ys;        // its unwrapped index xa - 1 .. xb: names its ring slot
};
template <bool GH> struct BandWalk {
    int xa, xb, nl, R, rb;
    bool rev;
    int xhm, xhp;          // the x-halo lines (mod X)
    const double *ghost;   // [2][m + 2][L], filled by k_ghost_unpack
    int m, L;
    __device__ __forceinline__ BandWalk(const BandK &a, int b, int J)
        : R((int)gridDim.x / a.H_parts), rb(b / a.H_parts), ghost(GH ? a.ghost : nullptr), m(a.m), L(a.L) {
        const int X = a.X;
        xa = (int)((int64_t)rb * X / R);
        xb = (int)((int64_t)(rb + 1) * X / R);
        nl = xb - xa;
        xhm = xa == 0 ? X - 1 : xa - 1;
        xhp = xb == X ? 0 : xb;
        rev = ((a.opt & BAND_ALT) && (rb & 1)) != ((a.opt & BAND_SERP) && (J & 1));
    }
    // the line iteration it updates
    __device__ __forceinline__ BandLine line(int it) const {
        if (rev) return {it == 0 ? xhp : (it == nl + 1 ? xhm : xb - it), it == 0 ? 2 : (it == nl + 1 ? 1 : 0), xb - it};
        return {it == 0 ? xhm : (it == nl + 1 ? xhp : xa - 1 + it), it == 0 ? 1 : (it == nl + 1 ? 2 : 0), xa - 1 + it};
    }
    // the owned line whose SpMV and dots iteration it (>= 2) runs
    __device__ __forceinline__ int spmv_line(int it) const { return rev ? xb + 1 - it : xa - 2 + it; }
    // ring offset of the line with unwrapped index ys (xa - 1 .. xb)
    __device__ __forceinline__ int slot(int ys) const { return ((ys - xa + 1) & 3) * BAND_T; }
    // a rank's first / last line range: the x-halo line of that kind is a neighbour rank's line
    __device__ __forceinline__ bool is_ghost(int kind) const {
        return GH && ghost && ((kind == 1 && rb == 0) || (kind == 2 && rb == R - 1));
    }
    // ... whose V_k (k < j), w_j and w_{j-1} arrived in the ghost buffer (slots k, wj_slot, wm_slot of
    // L doubles; v_0 in slot 0 at j = 0); null: the line is local
    __device__ __forceinline__ const double *ghost_line(int kind) const {
        return is_ghost(kind) ? ghost + (size_t)(kind == 1 ? 0 : 1) * (m + 2) * L : nullptr;
    }
    __device__ __forceinline__ int wj_slot(int j) const { return m + (j & 1); }
    __device__ __forceinline__ int wm_slot(int j) const { return j == 0 ? 0 : m + ((j + 1) & 1); }
};

// ---- operand loads and the DMA prefetch ----------------------------------------------------
// the SpMV operands of a line on the lane's row: D and m, and the line's v -+ 1 couplings
struct BandRowOp {
    double drow = 0.0, mrow = 1.0, tv0 = 0.0, tv1 = 0.0;
};
// update operands of an iteration's line on the lane's row: V_k (k < j), w_{j-1} (j = 0: v_0), w_j; SPF: + op
template <int J> struct BandLd {
    double v[J > 0 ? J : 1];
    double wm, wj;
    BandRowOp op;
};
// Software pipeline (J <= BAND_PF, as the registers allow): the kernel loads the next line's
// update operands during this line's SpMV and dots.  (A partial prefetch of 4 basis rows for
// larger J measured slower: 1234 vs 1254 it/s, spills; round 6: the prefetch for every J --
// spilling a few values past BAND_PF -- measured j13 758 -> 755, j16 880 -> 944, j18 989 -> 1087
// us in process; not kept)
template <int J, bool SPF, bool ND, bool GH>
__device__ __forceinline__ void band_load(const BandK &a, const BandWalk<GH> &W, const BandLane &T, int it,
                                          const BandLine &ln, BandLd<J> &o) {
    constexpr int j = J;
    const int L = T.L, v = T.v;
    if constexpr (SPF) {
        // the SpMV line of iteration it (owned when it >= 2): D, m on the lane's row, the line's
        // v couplings (the same loads band_spmv_operands issues without SPF)
        o.op = BandRowOp{};
        if (it >= 2) {
            const int xs = W.spmv_line(it);
            const int64_t rs = (int64_t)xs * L + (T.own ? v : T.v0);
            if (T.own) {
                if constexpr (!ND) o.op.drow = __builtin_nontemporal_load(a.lsv + rs);
                o.op.mrow = __builtin_nontemporal_load(a.mtri + rs);
            }
            o.op.tv0 = a.lsv[a.n + 2 * L + xs];
            o.op.tv1 = a.lsv[a.n + 2 * L + T.X + xs];
        }
    }
    const int64_t row = (int64_t)ln.y * L + (T.upd ? v : 0);
    o.wm = 0.0;
    o.wj = 0.0;
    const double *gh = W.ghost_line(ln.kind);
    if (T.upd) {
        if (gh) {
            o.wj = gh[(size_t)W.wj_slot(j) * L + v];
            o.wm = gh[(size_t)W.wm_slot(j) * L + v];
        } else {
            o.wj = __builtin_nontemporal_load(a.w_in + row);
            o.wm = __builtin_nontemporal_load((j == 0 ? a.V : a.w_prev) + row);
        }
    }
    if (gh) {
#pragma unroll
        for (int k = 0; k < J; ++k) o.v[k] = T.upd ? gh[(size_t)k * L + v] : 0.0;
    } else {
        // one lane pointer stepped by ld (per-k scalar bases would spill SGPRs: readlanes)
        const double *pv = a.V + row;
#pragma unroll
        for (int k = 0; k < J; ++k) {
            o.v[k] = T.upd ? __builtin_nontemporal_load(pv) : 0.0;
            pv += a.ld;
        }
    }
}

// BAND_L2PF: touch the rows iteration itp reads (its line's rows v0 - 1 .. v0 + LP of the J basis
// vectors, w_j and w_{j-1} (v_0 at j = 0); D and m of its SpMV line; ND: m only) by LDS-DMA loads
// (global_load_lds_dword, one lane per 128-B segment, into a scratch word nobody reads), the
// rows spread over the waves.  Ghost lines come from the ghost buffer: skipped
template <int J, bool CANON, bool ND, bool GH>
__device__ __forceinline__ void band_l2_prefetch(const BandK &a, const BandWalk<GH> &W, const BandLane &T, int itp,
                                                 int *pf_sink) {
    constexpr int j = J, PF_ROWS = J + 2 + (CANON ? (ND ? 1 : 2) : 0);
    if (itp > W.nl + 1) return;
    const BandLine ln = W.line(itp);
    const bool ghostl = W.is_ghost(ln.kind);
    const int xs = W.spmv_line(itp);   // its SpMV line (owned when itp >= 2)
    const int L = T.L, v0 = T.v0;
    const int vlo = v0 > 0 ? v0 - 1 : 0, vhi = v0 + T.LP < L ? v0 + T.LP + 1 : L;
    // (round 6: capping the prefetch at 10 basis rows -- a line's J + 4 rows of ~3.3 KB per
    // workgroup, 64 workgroups per XCD, overflow the 4 MB L2 past ~14 rows: PMC fetch 1.07x at
    // j = 13, 1.19x at j = 18 -- made j13-j18 11-33 us slower in process: not kept)
    for (int r = T.wv; r < PF_ROWS; r += BAND_W) {   // wave-uniform
        const double *vec;
        int64_t r0, r1;
        if (r < J + 2) {
            if (ghostl) continue;
            vec = r < J ? a.V + (size_t)r * a.ld : (r == J ? a.w_in : (j == 0 ? a.V : a.w_prev));
            r0 = (int64_t)ln.y * L + vlo;
            r1 = (int64_t)ln.y * L + vhi;
        } else {
            if (itp < 2) continue;
            vec = (r == J + 2 && !ND) ? a.lsv : a.mtri;
            r0 = (int64_t)xs * L + v0;
            r1 = r0 + T.LP;
        }
        const int64_t s0 = r0 >> 4, ns = ((r1 - 1) >> 4) - s0 + 1;   // 16 doubles = 128 B
        if (T.lane < ns)
            __builtin_amdgcn_global_load_lds(vec + ((s0 + T.lane) << 4), (__attribute__((address_space(3))) void *)pf_sink,
                                             4, 0, 0);
    }
}

// ---- 1. the update -------------------------------------------------------------------------
// the step's scalars; cs / ce / cp: s_k, e_k and the previous step's e'_k in LDS
struct BandCoef {
    const double *cs, *ce, *cp;
    double rinv, qc, ej, qp;
};
// p_j as step j-1's update formed it, then k_dc_update's operations; stores v_j on owned lines
// (and p_{j+1} at the last band step); vreg = V_k, v_j; returns p_{j+1}
template <int J>
__device__ __forceinline__ double band_update(const BandK &a, const BandLane &T, const BandCoef &c, const BandLine &ln,
                                              const BandLd<J> &o, double (&vreg)[J + 1]) {
    constexpr int j = J;
    const int64_t row = (int64_t)ln.y * T.L + (T.upd ? T.v : 0);
#pragma unroll
    for (int k = 0; k < J; ++k) vreg[k] = o.v[k];
    double pj = o.wm;   // j = 0: p_0 = v_0
    if (j >= 1) {
        double tp = o.wm;
#pragma unroll
        for (int k = 0; k < J; ++k) tp = band_msub(tp, c.cp[k], vreg[k]);
        pj = tp * c.qp;
    }
    double av = pj, tv = o.wj;
#pragma unroll
    for (int k = 0; k < J; ++k) {
        const double sk = c.cs[k], ek = c.ce[k];
        av = band_msub(av, sk, vreg[k]);
        tv = band_msub(tv, ek, vreg[k]);
    }
    double vj = pj;
    if (j >= 1) vj = av * c.rinv;
    tv = band_msub(tv, c.ej, vj);
    const double pn = tv * c.qc;
    vreg[J] = vj;
    if (ln.kind == 0 && T.own) {
        if (j >= 1) {
            st_wt(a.V + (size_t)j * a.ld + row, vj);
        }
        if (j == a.m - 2) st_wt(a.V + (size_t)(j + 1) * a.ld + row, pn);
    }
    return pn;
}

// ---- 2. the SpMV ---------------------------------------------------------------------------
// coded rows (VMODE 0 / 1): the lane's code word, the dictionary entry it holds for its wave
// and (VMODE 0) the SELL values
template <int WU, bool LSV> struct BandCodes {
    uint32_t word = 0u;
    int dv = 0;
    double d[LSV ? 1 : WU];
};
// the SpMV operands of line x loaded at the head of its iteration (no SPF; independent of the update):
// codes, dictionary (q, q0: the 64-row chunks of the lane's row and of its wave's first row), values, m
__device__ __forceinline__ int64_t band_chunk0(const BandLane &T, int64_t lrow) { return (lrow + T.v0 - BAND_OFF + 64 * T.wv) >> 6; }
template <int WU, int VMODE, bool ND>
__device__ __forceinline__ void band_spmv_operands(const BandK &a, const BandLane &T, int x, int64_t lrow, int64_t row,
                                                   BandRowOp &op, BandCodes<WU, (VMODE >= 1)> &cd) {
    constexpr bool LSV = VMODE >= 1, CANON = VMODE == 2;
    const int64_t q = row >> 6, q0 = band_chunk0(T, lrow);
    const int l64 = (int)(row & 63);
    if constexpr (!CANON) {
        cd.word = __builtin_nontemporal_load(a.pk + q * 64 + l64);
        const int64_t qd = q0 + (T.lane >> 4);
        cd.dv = (T.lane < 32 && qd >= 0 && qd * 64 < a.n) ? a.dict[qd * 16 + (T.lane & 15)] : 0;
    }
    if constexpr (LSV) {
        if constexpr (!ND) {
            if (T.own) op.drow = __builtin_nontemporal_load(a.lsv + row);
        }
        op.tv0 = a.lsv[a.n + 2 * T.L + x];
        op.tv1 = a.lsv[a.n + 2 * T.L + T.X + x];
    } else {
#pragma unroll
        for (int k = 0; k < WU; ++k) cd.d[k] = __builtin_nontemporal_load(a.val + q * 64 * WU + 64 * k + l64);
    }
    if (T.own) op.mrow = __builtin_nontemporal_load(a.mtri + row);
}

// canonical rows (VMODE 2): the row sum of line x from the ring in the line's stored order
// (canon_row_sum: every lane reads its five operands, a clamped row off its own rows), the
// in-block v -+ 1 couplings for the BJ solve in sub / sup, p on the lane's row in pc.
// BAND_ND: y = C p (no diagonal term; vtk_internal.hpp)
template <bool ND, bool GH>
__device__ __forceinline__ double band_spmv_canon(const BandK &a, const BandWalk<GH> &W, const BandLane &T,
                                                  const double *ring, int x, double tx0, double tx1, const BandRowOp &op,
                                                  double &sub, double &sup, double &pc) {
    // the line's stored order of the five kinds (the same for every lane of the line)
    int64_t cxm, cxp;
    const int ord = __builtin_amdgcn_readfirstlane(
        canon_order_xv(x, 0, a.n, T.L, T.X, GH && a.ghost ? a.left_blk : -1, cxm, cxp, a.xord));
    const int vv = T.own ? T.v : T.v0;
    const int sx = W.slot(x) - T.v0 + BAND_OFF;   // ring offset of line x
    const double t0 = tx0 * ring[W.slot(x - 1) - T.v0 + BAND_OFF + vv];
    const double t4 = tx1 * ring[W.slot(x + 1) - T.v0 + BAND_OFF + vv];
    pc = ring[sx + vv];
    const double t2 = op.drow * pc;
    const double t1 = op.tv0 * ring[sx + vv - 1];
    const double t3 = op.tv1 * ring[sx + vv + 1];
    const bool h1 = vv > 0, h3 = vv < T.L - 1;
    const double sa = canon_row_sum<ND>(ord, t0, t1, t2, t3, t4, h1, h3, T.ii);
    sub = (T.own && h1 && T.ii > 0) ? 0.0 + op.tv0 : 0.0;
    sup = (T.own && h3 && T.ii < 7) ? 0.0 + op.tv1 : 0.0;
    return T.own ? sa : 0.0;
}

// coded rows (VMODE 0 / 1): the SELL entries of the lane's row in stored order, gathers from the ring
template <int WU, bool LSV, bool GH>
__device__ __forceinline__ double band_spmv_coded(const BandK &a, const BandWalk<GH> &W, const BandLane &T,
                                                  const double *ring, int x, int64_t lrow, int64_t row, double tx0,
                                                  double tx1, const BandRowOp &op, const BandCodes<WU, LSV> &cd,
                                                  double &sub, double &sup) {
    const int L = T.L, v = T.v;
    const int sel = (int)((row >> 6) - band_chunk0(T, lrow)) * 16;
    const int wrapL = (T.X - 1) * L;   // |column - row| of a periodic x-coupling across the wrap
    double sacc = 0.0;
#pragma unroll
    for (int k = 0; k < WU; ++k) {
        const int code = (int)((cd.word >> (4 * k)) & 15u);
        const int off = __shfl(cd.dv, (sel + code) & 63, 64);
        if (T.own && code != PK_CODES) {
            // the column's line relative to x and its position in that line, by range
            // tests (vtk_csr_set_line_band checked: lines x-1..x+1, or the periodic wrap)
            const int t = v + off;
            int rel, vc;
            const int c = x * L + t;
            if (a.ghost && c >= (int)a.n) {   // halo column: a neighbour rank's line
                const int kk = c - (int)a.n, blk = kk >= L ? 1 : 0;
                rel = blk == a.left_blk ? -1 : 1;
                vc = kk - blk * L;
            } else if (t >= 0 && t < L) { rel = 0; vc = t; }
            else if (t >= L && t < 2 * L) { rel = 1; vc = t - L; }
            else if (t < 0 && t >= -L) { rel = -1; vc = t + L; }
            else if (t >= L) { rel = -1; vc = t - wrapL; }   // column in line X-1, row in line 0
            else { rel = 1; vc = t + wrapL; }                // column in line 0, row in line X-1
            const double xv = ring[W.slot(x + rel) + vc - T.v0 + BAND_OFF];
            double dk;
            if constexpr (LSV) dk = rel != 0 ? (rel > 0 ? tx1 : tx0) : (vc == v ? op.drow : (vc > v ? op.tv1 : op.tv0));
            else dk = cd.d[k];
            sacc += dk * xv;
            if (off == -1 && T.ii > 0) sub = sub + dk;
            if (off == 1 && T.ii < 7) sup = sup + dk;
        }
    }
    return sacc;
}

// ---- 3. the dots ---------------------------------------------------------------------------
// dots of the part's rows of one line: wave wv owns items wv, wv + 7, wv + 14 (item k <= j: s_k,
// z_k; j + 1: |p|^2, p.w, |w|^2), lanes stride the rows.  Items outer: each item's loop streams
// one basis row (vbuf) against p (pr: the line's ring slot) and w (wbuf) (rows outer with p, w
// read once per row for all items measured slower: 1268-1285 vs 1296 it/s)
template <int J>
__device__ __forceinline__ void band_dots(const BandLane &T, const double *pr, const double *vbuf, const double *wbuf,
                                          double (&acc)[band_items<J>()][3]) {
    constexpr int j = J;
#pragma unroll
    for (int u = 0; u < band_items<J>(); ++u) {
        const int itm = T.wv + BAND_W * u;
        if (itm <= j) {
            const double *vk = vbuf + itm * BAND_LP;
#pragma unroll VTK_BAND_DOTS_UNROLL
            for (int t = T.lane; t < T.LP; t += 64) {
                const double vv = vk[t];
                acc[u][0] = band_madd(acc[u][0], vv, pr[t]);
                acc[u][1] = band_madd(acc[u][1], vv, wbuf[t]);
            }
        } else if (itm == j + 1) {
#pragma unroll VTK_BAND_DOTS_UNROLL
            for (int t = T.lane; t < T.LP; t += 64) {
                const double pv = pr[t], wq = wbuf[t];
                acc[u][0] = band_madd(acc[u][0], pv, pv);
                acc[u][1] = band_madd(acc[u][1], pv, wq);
                acc[u][2] = band_madd(acc[u][2], wq, wq);
            }
        }
    }
}

// per-workgroup partials (slot b) in launch_dc_dots' layout for step j+1
template <int J>
__device__ __forceinline__ void band_write_partials(const BandK &a, const BandLane &T, int b,
                                                    const double (&acc)[band_items<J>()][3], double *red) {
    constexpr int j = J;
#pragma unroll
    for (int u = 0; u < band_items<J>(); ++u) {
        const int itm = T.wv + BAND_W * u;
        if (itm <= j + 1) {   // wave-uniform
            const double t0 = wave_allsum(acc[u][0]), t1 = wave_allsum(acc[u][1]), t2 = wave_allsum(acc[u][2]);
            if (T.lane == 0) {
                if (itm <= j) {
                    red[itm] = t0;
                    red[DC_MAXJ + itm] = t1;
                } else {
                    red[2 * DC_MAXJ] = t0;
                    red[2 * DC_MAXJ + 1] = t1;
                    red[2 * DC_MAXJ + 2] = t2;
                }
            }
        }
    }
    __syncthreads();
    const int jn = j + 1;
    for (int qq = T.tid; qq < DC_NQ; qq += BAND_T) {
        const bool used = qq < jn || (qq >= DC_MAXJ && qq < DC_MAXJ + jn) || qq >= 2 * DC_MAXJ;
        if (used) a.part[(size_t)qq * GMAX + b] = red[qq];
    }
}

// ---- the kernel ----------------------------------------------------------------------------
template <int WU, int J, int VMODE = 0, bool GH = true, int OPT = 0>
__global__ __launch_bounds__(BAND_T) __attribute__((amdgpu_waves_per_eu(band_wpe<OPT>()))) void k_band_step(BandK a) {
    __shared__ double vbuf[(J + 1) * BAND_LP];   // the basis rows of the line updated last (the dots')
    __shared__ double ring[4 * BAND_T];          // p_{j+1} of four lines
    __shared__ double wbuf[BAND_LP];
    __shared__ double red[DC_NQ];
    __shared__ double cs[BAND_JV], ce[BAND_JV], cp[BAND_JV];
    __shared__ int pf_sink[64];   // L2PF: the DMA's destination (never read)
    constexpr int j = J;
    constexpr bool LSV = VMODE >= 1, CANON = VMODE == 2, ND = CANON && (OPT & BAND_ND);
    constexpr bool PF = J <= BAND_PF, SPF = PF && CANON && (OPT & BAND_SPF), L2PF = (OPT & BAND_L2PF) != 0;
    if (__builtin_nontemporal_load(&a.st->xup_tag) == j) {   // the cycle's x update
        dc_xupdate_body<BAND_XUP_XB, true>(a.V, a.ld, j, __builtin_nontemporal_load(&a.st->stop_col), a.n, a.cf, a.x,
                                           a.H, a.S, a.m, a.w_prev);
        return;
    }
    if (stopped(&a.st->stop_col, j)) return;
    const int b = band_block(a.opt, a.H_parts);
    const BandLane T(a, b % a.H_parts);
    const BandWalk<GH> W(a, b, J);
    // LSV: the lane's x-coupling values (position v in every line)
    double tx0 = 0.0, tx1 = 0.0;
    if constexpr (LSV) {
        if (T.v >= 0 && T.v < T.L) {
            tx0 = a.lsv[a.n + T.v];
            tx1 = a.lsv[a.n + T.L + T.v];
        }
    }
    for (int k = T.tid; k < j; k += BAND_T) {
        cs[k] = a.cf->s[k];
        ce[k] = a.cf->e[k];
        cp[k] = a.cf->e_prev[k];
    }
    const BandCoef coef{cs, ce, cp, a.cf->rinv, a.cf->q, a.cf->e[j], a.cf->q_prev};
    band_sync<OPT>();
    double vreg[J + 1];
    double acc[band_items<J>()][3];
#pragma unroll
    for (int u = 0; u < band_items<J>(); ++u) acc[u][0] = acc[u][1] = acc[u][2] = 0.0;
    BandLd<J> nx;
    if constexpr (PF) band_load<J, SPF, ND>(a, W, T, 0, W.line(0), nx);
    if constexpr (L2PF) band_l2_prefetch<J, CANON, ND>(a, W, T, PF ? 1 : 0, pf_sink);
    for (int it = 0; it <= W.nl + 1; ++it) {
        const BandLine ln = W.line(it);   // the line updated now
        const int x = W.spmv_line(it);    // the line whose SpMV and dots run now (owned when it >= 2)
        const bool work = it >= 2;
        const int64_t lrow = (int64_t)(work ? x : W.xa) * T.L, row = lrow + (T.own ? T.v : T.v0);
        BandRowOp op;
        BandCodes<WU, LSV> cd;
        if (work && !SPF) band_spmv_operands<WU, VMODE, ND>(a, T, x, lrow, row, op, cd);
        // 1. update of line ln.y; the next iteration's operands (PF) and the DMA prefetch behind it
        {
            BandLd<J> cu;
            if constexpr (PF) cu = nx;
            else band_load<J, SPF, ND>(a, W, T, it, ln, cu);
            if constexpr (SPF) op = cu.op;
            const double pn = band_update<J>(a, T, coef, ln, cu, vreg);
            if (T.upd) ring[W.slot(ln.ys) + T.tid] = pn;
            if constexpr (PF) {
                if (it <= W.nl) band_load<J, SPF, ND>(a, W, T, it + 1, W.line(it + 1), nx);
            }
            if constexpr (L2PF) band_l2_prefetch<J, CANON, ND>(a, W, T, PF ? it + 2 : it + 1, pf_sink);
        }
        band_sync<OPT>();
        if (work) {
            // 2. w = M^-1 A p_{j+1} on the part's rows of line x, gathers from the ring
            double sacc, sub = 0.0, sup = 0.0;
            double pc = 0.0;   // ND: p on the lane's row
            if constexpr (CANON) sacc = band_spmv_canon<ND>(a, W, T, ring, x, tx0, tx1, op, sub, sup, pc);
            else sacc = band_spmv_coded<WU, LSV>(a, W, T, ring, x, lrow, row, tx0, tx1, op, cd, sub, sup);
            double z = bj_trim_group<8>(T.own ? sacc : 0.0, T.lane, sub, sup, op.mrow);
            if constexpr (ND) z = pc + z;   // w = p + M^-1 (C p)
            if (T.own) {
                st_wt(a.w_out + row, z);
                wbuf[T.tid - BAND_OFF] = z;
            }
            band_sync<OPT>();
            // 3. dots of the part's rows of line x
            band_dots<J>(T, ring + W.slot(x) + BAND_OFF, vbuf, wbuf, acc);
            band_sync<OPT>();
        }
        if (it >= 1 && it <= W.nl && T.own) {   // line ln.y is owned: its basis rows for the dots one line on
#pragma unroll
            for (int k = 0; k <= J; ++k) vbuf[k * BAND_LP + T.tid - BAND_OFF] = vreg[k];
        }
    }
    band_write_partials<J>(a, T, b, acc, red);
}

// ---- the launch table ----------------------------------------------------------------------
// SPF only at the step indices where it measured faster: in-process A/B, round 6, on the final
// kernels (profiles/r06_band_bits_ab.json): j = 0 -12 us, j = 3, 4 -3 us each at C3; j = 1, 2
// +2 / +5 us, j = 6-12 +6 ... +20 us each (the operands' registers held across the SpMV + dots);
// the same signs on C2 and the C3 slabs
constexpr bool band_spf_j(int J) { return J == 0 || J == 3 || J == 4; }
// The compile-time variant (OPT) of the canonical-row kernel of step J for the run-time bits opt
// (after band_spf_j's mask), one rank (GH false) or across ranks: the same variants either way --
// until round 6 the distributed band step ran OPT 0 only, which the one-rank slab projections
// (--comm-solo: no ghost lines) did not see.
//   J > BAND_PF: L2PF where the registers hold no next line (in-process A/B, C3, round 6: j13-j17
//     745-925 -> 709-875 us, j18 991 -> 970; with the register prefetch (J <= 12, two lines ahead)
//     it cost 11-35 us per launch).  Its instantiation carries SPF's bit, inert there.
//   J <= BAND_J3: WPC3, only where the LDS of three workgroups fits.
constexpr int band_variant(int J, bool GH, int opt) {
    const int nd = opt & BAND_ND;
    if (J > BAND_PF && (opt & BAND_L2PF)) return BAND_L2PF | BAND_SPF | nd;
    if (J <= BAND_J3 && (opt & BAND_WPC3)) return (opt & (BAND_SPF | BAND_WPC3)) | nd;
    if (GH && J <= BAND_J3) return nd;   // asymmetry: SPF without WPC3 at J <= BAND_J3 is SPF on one rank, plain across ranks
    if (GH && J > BAND_PF) return nd;    // asymmetry: SPF alone at J > BAND_PF, one rank only -- band_spf_j clears it: cannot occur
    return (opt & BAND_SPF) | nd;
}
// whether some opt maps to variant V at (J, GH): only those variants are instantiated
constexpr bool band_has(int J, bool GH, int V) {
    for (int opt = 0; opt < 2 * BAND_ND; ++opt)
        if (band_variant(J, GH, opt) == V) return true;
    return false;
}
// canonical rows, one rank (GH false) or across ranks (the ghost lines' update operands come from the ghost buffer)
template <int J, bool GH> static void launch_band_canon(BandK a, int grid, hipStream_t s) {
    if (!band_spf_j(J)) a.opt &= ~BAND_SPF;
    const int v = band_variant(J, GH, a.opt);
    const dim3 g(grid), blk(BAND_T);
#define VTK_BAND_V(V_)                                                            \
    if constexpr (band_has(J, GH, V_)) {                                          \
        if (v == (V_)) {                                                          \
            hipLaunchKernelGGL((k_band_step<5, J, 2, GH, V_>), g, blk, 0, s, a);  \
            return;                                                               \
        }                                                                         \
    }
    VTK_BAND_V(0) VTK_BAND_V(BAND_SPF) VTK_BAND_V(BAND_WPC3) VTK_BAND_V(BAND_SPF | BAND_WPC3) VTK_BAND_V(BAND_SPF | BAND_L2PF)
    VTK_BAND_V(BAND_ND) VTK_BAND_V(BAND_ND | BAND_SPF) VTK_BAND_V(BAND_ND | BAND_WPC3)
    VTK_BAND_V(BAND_ND | BAND_SPF | BAND_WPC3) VTK_BAND_V(BAND_ND | BAND_SPF | BAND_L2PF)
#undef VTK_BAND_V
}
// step J's four forms: SELL values and codes, table values with codes, canonical rows on one rank / across ranks
template <int J> static void launch_band_j(const BandK &a, int grid, hipStream_t s) {
    if (!a.lsv) hipLaunchKernelGGL((k_band_step<5, J>), dim3(grid), dim3(BAND_T), 0, s, a);
    else if (!a.canon) hipLaunchKernelGGL((k_band_step<5, J, 1>), dim3(grid), dim3(BAND_T), 0, s, a);
    else if (a.ghost) launch_band_canon<J, true>(a, grid, s);
    else launch_band_canon<J, false>(a, grid, s);
}

hipError_t launch_band_step(const BandK &a, int grid, int wu, hipStream_t s) {
    // X < 2 with ghost lines: the one slab with the stored order canon_row_sum does not have (vtk_device.hpp)
    if (wu != 5 || a.H_parts < 1 || a.L % a.H_parts != 0 || a.L / a.H_parts > BAND_LP || (a.L / a.H_parts) % 8 != 0 ||
        a.j + 1 > BAND_JV || grid < a.H_parts || grid > GMAX || grid % a.H_parts != 0 || grid / a.H_parts > a.X ||
        a.n > INT32_MAX / 2 || (a.ghost && a.X < 2))
        return hipErrorInvalidValue;
    switch (a.j) {
#define VTK_BAND_J(J_) case J_: launch_band_j<J_>(a, grid, s); break;
        VTK_BAND_J(0) VTK_BAND_J(1) VTK_BAND_J(2) VTK_BAND_J(3) VTK_BAND_J(4) VTK_BAND_J(5) VTK_BAND_J(6)
        VTK_BAND_J(7) VTK_BAND_J(8) VTK_BAND_J(9) VTK_BAND_J(10) VTK_BAND_J(11) VTK_BAND_J(12) VTK_BAND_J(13)
        VTK_BAND_J(14) VTK_BAND_J(15) VTK_BAND_J(16) VTK_BAND_J(17) VTK_BAND_J(18)
#undef VTK_BAND_J
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ghost exchange of the distributed band step: pack the rank's first / last line
// of v_{j-1} (V[j-1]; V[0] at j = 0) and w_j into send pieces of BAND_GHOST_VECS L, unpack the
// received pieces into the ghost slots (v_{j-1} -> slot j-1, v_0 -> slot 0 at j = 0, w_j ->
// m + (j & 1): step j-1's w stays in the other slot for the recompute of p_j)
__global__ __launch_bounds__(NT) void k_ghost_pack(const double *__restrict__ V, int64_t ld, int j,
                                                   const double *__restrict__ w, int64_t n, int L,
                                                   double *__restrict__ sbuf, int64_t off_first, int64_t off_last) {
    constexpr int NV = BAND_GHOST_VECS;
    for (int i = blockIdx.x * NT + threadIdx.x; i < 2 * NV * L; i += gridDim.x * NT) {
        const int side = i / (NV * L), r = i % (NV * L), vec = r / L, t = r % L;
        const int64_t off = side == 0 ? off_first : off_last;
        if (off < 0) continue;
        const int64_t row = (side == 0 ? 0 : n - L) + t;
        sbuf[off + r] = vec == 0 ? V[(size_t)(j >= 1 ? j - 1 : 0) * ld + row] : w[row];
    }
}

__global__ __launch_bounds__(NT) void k_ghost_unpack(const double *__restrict__ rbuf, int64_t off_left, int64_t off_right,
                                                     int j, int m, int L, double *__restrict__ ghost) {
    constexpr int NV = BAND_GHOST_VECS;
    for (int i = blockIdx.x * NT + threadIdx.x; i < 2 * NV * L; i += gridDim.x * NT) {
        const int side = i / (NV * L), r = i % (NV * L), vec = r / L, t = r % L;
        const int64_t off = side == 0 ? off_left : off_right;
        if (off < 0) continue;
        const int slot = vec == 0 ? (j >= 1 ? j - 1 : 0) : m + (j & 1);
        ghost[((size_t)side * (m + 2) + slot) * L + t] = rbuf[off + r];
    }
}

hipError_t launch_ghost_pack(const double *V, int64_t ld, int j, const double *w, int64_t n, int L, double *sbuf,
                             int64_t off_first, int64_t off_last, hipStream_t s) {
    hipLaunchKernelGGL(k_ghost_pack, dim3((2 * BAND_GHOST_VECS * L + NT - 1) / NT), dim3(NT), 0, s, V, ld, j, w, n, L, sbuf, off_first,
                       off_last);
    return hipGetLastError();
}

hipError_t launch_ghost_unpack(const double *rbuf, int64_t off_left, int64_t off_right, int j, int m, int L,
                               double *ghost, hipStream_t s) {
    hipLaunchKernelGGL(k_ghost_unpack, dim3((2 * BAND_GHOST_VECS * L + NT - 1) / NT), dim3(NT), 0, s, rbuf, off_left, off_right, j, m, L,
                       ghost);
    return hipGetLastError();
}

// distributed form of the check (local column numbering; the halo is exactly two neighbour lines,
// halo block lblk the left one): an owned column within lines x-1..x+1 of the row's line without
// wrap, a halo column only from the first (left block) or last (right block) local line
__global__ __launch_bounds__(NT) void k_band_check_dist(const int32_t *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices, int64_t n, int L,
                                                        int lblk, int *bad) {
    const int64_t X = n / L;
    for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (int64_t)gridDim.x * NT) {
        const int64_t x = r / L, vr = r % L;
        bool ok = true, vloc = true;
        for (int k = indptr[r]; k < indptr[r + 1]; ++k) {
            const int64_t c = indices[k];
            int64_t vc;
            if (c < 0 || c >= n + 2 * L) { ok = false; break; }
            if (c < n) {
                const int64_t rel = c / L - x;
                if (rel < -1 || rel > 1) { ok = false; break; }
                vc = c % L;
            } else {
                const int64_t kk = c - n, blk = kk / L;
                if ((blk == lblk && x != 0) || (blk != lblk && x != X - 1)) { ok = false; break; }
                vc = kk % L;
            }
            if (vc - vr < -1 || vc - vr > 1) vloc = false;
        }
        if (!ok) atomicOr(bad, 1);
        if (!vloc) atomicOr(bad, 2);
    }
}

hipError_t launch_band_check_dist(const int32_t *indptr, const int32_t *indices, int64_t n, int L, int lblk, int *bad,
                                  hipStream_t s) {
    int64_t g = (n + NT - 1) / NT;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_band_check_dist, dim3((unsigned)g), dim3(NT), 0, s, indptr, indices, n, L, lblk, bad);
    return hipGetLastError();
}

// *bad |= 1 when a column lies outside lines x-1..x+1 (mod X) of its row's line x; |= 2 when it
// lies more than one row off the row's position v within its line
__global__ __launch_bounds__(NT) void k_band_check(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                   int64_t n, int L, int X, int *bad) {
    for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < n; r += (int64_t)gridDim.x * NT) {
        const int64_t x = r / L, vr = r % L;
        bool ok = true, vloc = true;
        for (int k = indptr[r]; k < indptr[r + 1]; ++k) {
            const int64_t c = indices[k];
            if (c < 0 || c >= n) { ok = false; break; }
            int64_t rel = c / L - x;
            if (rel > 1) rel -= X;
            else if (rel < -1) rel += X;
            if (rel < -1 || rel > 1) { ok = false; break; }
            const int64_t dv = c % L - vr;
            if (dv < -1 || dv > 1) vloc = false;
        }
        if (!ok) atomicOr(bad, 1);
        if (!vloc) atomicOr(bad, 2);
    }
}

hipError_t launch_band_check(const int32_t *indptr, const int32_t *indices, int64_t n, int L, int X, int *bad,
                             hipStream_t s) {
    int64_t g = (n + NT - 1) / NT;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(k_band_check, dim3((unsigned)g), dim3(NT), 0, s, indptr, indices, n, L, X, bad);
    return hipGetLastError();
}

}  // namespace vtk
