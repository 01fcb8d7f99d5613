// vtk_gmres.cpp -- the restarted GMRES driver: host orchestration of the gfx950 kernels.
//
// The driver restates scipy.sparse.linalg.gmres (scipy/sparse/linalg/_isolve/iterative.py:
// 692-841) with every vector operation and every reduction on the device; the host only keeps
// SciPy's outer-loop bookkeeping (ptol_max_factor, :816-838) and reads back one 100-byte state
// record per restart cycle.  Inside a cycle the Givens rotations, the inner stop test
// (presid <= ptol, :794) and the breakdown test (:766) run on the device: kernels of columns
// after the stop column return at entry (GmresState::stop_col), so the host enqueues a cycle
// without a per-step round trip and throttles itself with events LOOKAHEAD columns behind.
#include <climits>

#include "vtk_driver.hpp"

using namespace vtk;

namespace {

struct Solver {
    vtk_csr *A;
    vtk_prec *M;
    vtk_ctx *c;
    int64_t n, ld;
    int m, G;
    const double *b = nullptr;
    double *x = nullptr;                         // the solution (the DCGS2 update pass may update it)
    double *V = nullptr, *w = nullptr, *tmp = nullptr, *r = nullptr, *H = nullptr, *S = nullptr, *giv = nullptr;
    double *part[4] = {};
    bool dc = false;
    double *Hraw = nullptr, *dcpart = nullptr;   // DCGS2
    DcCoef *cf = nullptr;
    // compressed basis (vtk_gmres_set_basis): the finalised columns in float32, the
    // candidates p_j in pc[j % 2]; V is null.  start(): where the cycle's start direction M^-1 r is written
    bool cb = false;
    float *Vc = nullptr;
    double *pc[2] = {};
    double *cand(int j) const { return cb ? pc[j & 1] : V + (size_t)j * ld; }
    double *start() const { return cand(0); }
    // line-band DCGS2 step (k_band_step): grid, parts per line; w rotates over s.w, s.tmp, w3
    // (step j's w in the buffer j % 3: the band step reads w_{j-1} and w_j, writes w_{j+1})
    bool band = false;
    int band_G = 0, band_H = 1;
    int band_G3 = 0;   // grid of the three-workgroups-per-CU launches (BAND_WPC3, j <= BAND_J3)
    // workgroups (= partials) of the band step launched at step j
    int band_grid(int j, int opt) const { return (opt & BAND_WPC3) && j <= BAND_J3 && band_G3 > 0 ? band_G3 : band_G; }
    double *w3 = nullptr;
    double *wbuf(int j) const { return j % 3 == 0 ? w : j % 3 == 1 ? tmp : w3; }
    double *ghost = nullptr, *gsend = nullptr, *grecv = nullptr;   // distributed band step
    // across ranks: the first launch of this rank that failed (Vote), and the fail_step test hook
    // still to fire in this solve
    Vote vote;
    bool fail_pending = false;
    // the cycle in flight: the device stop column, its host mirror, the throttle events
    const int *stop = nullptr;
    volatile int *mirror = nullptr;
    hipEvent_t *ev = nullptr;
    int ev_step[LOOKAHEAD + 1], nev = 0, synced = 0;   // throttle(): the recorded events' steps
};
#define SOFT(x) SOFT_LAUNCH(s.c, &s.vote, x)

// ---- path predicates ---------------------------------------------------------------------------

// the x-line ring with the solver's epilogues (k_lsv_ring_epi): one rank, line-separable canonical
// rows, their tables in use (tunings band_lsv, sell_canon), the tridiagonal BJ(8) when bj
// (across ranks: the slab's x-halo lines come from the two neighbour lines of the halo -- band_ghost --
// or, on a rank without neighbours, the one-rank wrap)
bool cyc_ring_ok(vtk_ctx *c, const vtk_csr *A, const vtk_prec *M, bool bj) {
    const bool solo = !c->dist || (A->n_halo == 0 && A->n_send == 0 && !A->band_ghost);
    if (c->tune.cyc_ring <= 0 || (!solo && !A->band_ghost) || !A->d_lsv || !A->lsv_canon || A->band_L <= 0 ||
        A->band_L % 8 != 0 || !c->tune.band_lsv || !c->tune.sell_canon || band_parts(A->band_L) < 1 ||
        A->n_local / A->band_L < (A->band_ghost ? 2 : 3))
        return false;
    return !bj || bj8_tri(M);
}

// the line path's table SpMV: the line-separable, canonical rows' tables (tunings band_lsv,
// sell_canon) of a uniform width-5 SELL copy; across ranks with the ghost lines
bool line_lsv_ok(vtk_ctx *c, const vtk_csr *A) {
    return A->d_lsv && A->band_L > 0 && c->tune.band_lsv && A->use_sell && A->sell.uniform_w == 5 && A->sell.d_pk &&
           A->sell.n_wide == 0 && (!c->dist || A->band_ghost);
}

// Band eligibility (line-band DCGS2 step: SELL of uniform width 5 with coded columns, no wide
// chunk, f64 values, tridiagonal BJ(8) -- the fused step's TRIM apply --, restart <= 20; tuning
// band 0 / vtk_gmres_set_band: off, tools/ab_env.py alternates it), in two parts.
// `possible`: the rank-uniform part -- band_L is set on all ranks or none; the orthogonalisation,
// the switch, the preconditioner and restart are the callers' uniform arguments.  run_gmres needs
// the ranks' agreement only when it holds.
// Returned: the rank-local rest (layout, current factors, geometry), with the geometry in s:
// parts per line (rows per workgroup <= 400; > 1 needs the v-locality of the couplings), two
// workgroups per CU, >= 2 lines per range (vtk_line_band_plan).
bool band_eligible(Solver &s, bool &possible) {
    vtk_ctx *c = s.c;
    const vtk_csr *A = s.A;
    const vtk_prec *M = s.M;
    possible = s.dc && c->tune.band && A->band_L > 0 && M && M->kind == VTK_PREC_BJACOBI && M->bs == 8 && s.m >= 2 && s.m <= 20;
    if (!possible || A->band_L % 8 != 0 || !(!c->dist || !A->band_ghost || c->comm || c->host_comm) ||
        !A->use_sell || A->sell.uniform_w != 5 || !A->sell.d_pk || A->sell.n_wide != 0 || A->fp32 || !bj_fused(M) || !bj8_tri(M))
        return false;
    vtk_band_geometry g{};
    if (vtk_line_band_plan(s.n, A->band_L, c->n_cu, &g) != VTK_OK || (g.parts > 1 && !A->band_vloc)) return false;
    s.band_H = g.parts;
    s.band_G = g.ranges * g.parts;
    // three workgroups per CU for the low-j steps: 1.5x the line ranges (>= 2 lines each)
    const int64_t R3 = std::min<int64_t>({std::max<int64_t>(1, 3LL * (c->n_cu > 0 ? c->n_cu : 256) / g.parts), g.lines / 2, (int64_t)GMAX / g.parts});
    s.band_G3 = (int)R3 * g.parts;
    return true;
}

// ---- the step plan: every path decision of a solve, made once (none can change within it) ------
struct StepPlan {
    bool g4_fits, g4_fused, g4_ring, wide9, ring4, fused;
    bool ring0;      // step 0 of a band cycle through the x-line ring
    bool split;      // interior / boundary pieces of the fused step (world > 1)
    bool line_dc, line2_step, linec_step, line_lsv, line_canon, line_fuse;
    bool neumann_step;   // the Neumann wrapper: SpMV, then its corrections (prec_apply)
    bool band_lsv, band_canon, band_nd;
    int band_opt;
    bool resid_fused, resid_g4, resid_ring;   // the cycle-end residual's kernel (residual())
    const Tiles *ft, *rtiles;
    double n8, b_csr, b_lsv, b_inv, b_band, b_solver;
    char jname[20][16];   // "band_step_jNN" (tuning prof_perj)
};

StepPlan step_plan(const Solver &s) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    vtk_prec *M = s.M;
    const int64_t n = s.n;
    StepPlan P{};
    P.n8 = 8.0 * n;
    // SpMV + BJ and the step's dots in one pass for BJ-fused tiles with bs <= 8 (larger blocks
    // would spill the fused kernel's registers)
    // ... except for rows wider than 8 (the 4D operator: 9 entries) without a halo to overlap:
    // there the SpMV + BJ kernel and the streaming dots kernel beat the register-capped fused
    // kernel (C4: 707 + 658 us vs 1473 us per step, 422 vs 405 it/s)
    // (with the 4D grid rows (Grid4) the fused kernel loads no values or codes: tuning c4_fused)
    P.g4_fits = A->d_g4tab && g4_ring_fits(A->g4, n, c->tune.g4_gr);
    P.g4_fused = A->d_g4tab && c->tune.grid4 && c->tune.c4_fused && (c->tune.g4_ring <= 0 || !P.g4_fits);   // C4 A/B: 213.8 -> 210.3 ms
    // grid rows with x staged through LDS (k_g4_ring) for the split step's SpMV + BJ
    P.g4_ring = g4_ring_ok(c, A, M);
    P.split = bj_split(M);
    P.wide9 = A->use_sell && A->sell.uniform_w > 8 && !P.split && !P.g4_fused;
    // the ring step also across ranks: interior groups while the halo planes
    // are in flight, the boundary planes' groups once they have landed
    P.ring4 = P.g4_ring && A->use_sell && A->sell.uniform_w > 8 && !P.g4_fused;
    // (the compressed basis keeps the dots of steps that read stored columns out of the operator step:
    // SpMV + BJ without dots, then the compressed dots kernel)
    P.fused = bj_fused(M) && M->bs <= 8 && !P.wide9 && !P.ring4 && !s.cb;
    P.ring0 = P.fused && s.band && cyc_ring_ok(c, A, M, true);
    // line Jacobi with segments <= 32 (register sweeps): dots fused into the sweep kernel
    P.line_dc = M && M->kind == VTK_PREC_LINE && M->line.seg >= 1 && M->line.seg <= 32 && s.G <= GMAX;
    // line product: SpMV, sweep 1 in place, sweep 2 with the dots (tuning line2_dc)
    P.line2_step = M && M->kind == VTK_PREC_LINE2 && M->line2.seg >= 1 && M->line2.seg <= 32 && s.G <= GMAX;
    // periodic whole lines: SpMV, the three apply phases, then the dots kernel
    P.linec_step = M && M->kind == VTK_PREC_LINEC && s.G <= GMAX;
    // the Neumann wrapper: SpMV, z_1, the corrections; the last one with the step's dots
    // where its kernel has that form (tuning neu_dc), else the dots kernel
    P.neumann_step = M && M->kind == VTK_PREC_NEUMANN && s.G <= GMAX;
    // line path on a line-separable operator: the SpMV from the tables (VTK_BAND_LSV=0: SELL)
    P.line_lsv = (P.line_dc || P.line2_step || P.linec_step) && line_lsv_ok(c, A);
    P.ft = M ? &M->tiles : &A->tiles;
    P.b_csr = matrix_bytes(A);
    P.b_lsv = P.b_csr - 8.0 * (double)A->sell.entries + 8.0 * (double)n;
    // canonical rows: the diagonal only (tuning sell_canon 0: the codes too; A/B)
    P.line_canon = P.line_lsv && A->lsv_canon && c->tune.sell_canon;
    // one rank: the SpMV inside the sweep kernel (y never stored)
    P.line_fuse = P.line_dc && P.line_canon && line_fuse_ok(c, A, M) && !s.cb;
    P.b_inv = prec_row_bytes(M) * n;
    P.b_solver = solver_matrix_bytes(A);
    // line-separable values in the band step (tuning band_lsv 0: the SELL values)
    P.band_lsv = s.band && A->d_lsv && c->tune.band_lsv;
    P.band_canon = c->tune.band_canon != 0;       // 0: read the codes anyway (A/B)
    // the band step's variant bits (BandOpt) exist for the line-separable, canonical-row
    // instantiations (one rank and, since round 6, across ranks with ghost lines): every
    // other launch, and the partial count its successor reads, takes the base grid
    // BAND_L2PF (the LDS-DMA prefetch of J > BAND_PF) and BAND_ALT (the alternating walk) pay only on long
    // basis vectors: on smaller ones (C2, the C3 slabs) more of the basis stays in the Infinity
    // Cache between steps, so the DMA's issue and L2 over-fetch cost more than the latency it hides
    // and the halo lines' second read hits anyway (band_long_rows, vtk_internal.hpp)
    // BAND_SERP (odd steps walk the other way round) stays at every size: in-process A/B 63 vs 31,
    // median ms per solve (spread of the eight SERP-off solves): C3 36.62 vs 37.37 (0.18), C3/2
    // slab 18.86 vs 18.95 (0.02), C2 10.21 vs 10.28 (0.08), C3/8 slab 6.16 vs 6.23 (0.04)
    // (profiles/serpentine_ab*.json)
    // BAND_ND (no read of the diagonal table, w = p + M^-1 (A - M) p) exists for the same
    // instantiations only: masked off with the others where the rows are not canonical line-separable
    P.band_opt = P.band_lsv && A->lsv_canon && P.band_canon
                     ? (n >= c->tune.band_long_rows ? c->tune.band_opt : c->tune.band_opt & ~(BAND_L2PF | BAND_ALT))
                     : 0;
    // the band step's matrix bytes: SELL codes + dictionary + (values: 8 B per row from D, or
    // the SELL values); with BAND_ND no matrix bytes per row at all
    P.band_nd = (P.band_opt & BAND_ND) != 0;
    P.b_band = P.band_lsv ? (A->lsv_canon && P.band_canon
                                 ? (P.band_nd ? 0.0 : 8.0 * (double)n)   // the diagonal only
                                 : P.b_csr - 8.0 * (double)A->sell.entries + 8.0 * (double)n)
                          : P.b_csr;
    // r = b - A x (iterative.py:737, :816).  When the BJ tiles allow (or M is the identity) the
    // residual kernel also applies M^-1 and writes v0's direction straight into V[0]: the next
    // cycle's psolve(r) (:742) is then already done.
    P.resid_fused = !M || bj_fused(M);
    P.rtiles = (M && bj_fused(M)) ? &M->tiles : &A->tiles;
    P.resid_g4 = P.resid_fused && P.g4_ring && A->sell.uniform_w > 8;   // 9-wide 4D grid rows: through k_g4_ring
    // the same through the x-line ring (fused: with the tridiagonal BJ(8))
    P.resid_ring = P.resid_fused ? M && cyc_ring_ok(c, A, M, true) : cyc_ring_ok(c, A, M, false);
    if (c->tune.prof_perj)
        for (int j = 0; j < 20; ++j) std::snprintf(P.jname[j], sizeof(P.jname[j]), "band_step_j%02d", j);
    return P;
}

// ---- the operator step w = M^-1 A p, one function per form; cnt: the partials it wrote (0: none)

// generic: w = M^-1 A v (fused when the tiles allow), partials: part[0] = w^2 (h0), part[1] = v0*w
int precond_matvec(Solver &s, const StepPlan &P, const double *v, double *w, int col, Red &h0, Red &d0, bool want_dots = true) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    const int *stop = s.stop;
    TRY(halo_exchange(A, v));
    const double *v0 = want_dots ? s.V : nullptr;
    const double n8 = P.n8, b_csr = P.b_solver, b_inv = P.b_inv;
    int cnt;
    if (!s.M) {
        Prof pf(c, "spmv_w", col, b_csr + 3 * n8);
        const SpmvIn in = lsv_in(spmv_in(A, &A->tiles, v), A);
        HIPCHK(c, launch_spmv(in, EPI_PREC, w, nullptr, BjOp{}, v0, s.part[0], s.part[1], stop, col, c->stream));
        cnt = spmv_grid(in);
    } else if (bj_fused(s.M)) {
        Prof pf(c, "spmv_bj", col, b_csr + b_inv + 3 * n8);   // x, v0, w + CSR + BJ rows
        const SpmvIn in = lsv_in(spmv_in(A, &s.M->tiles, v), A);
        HIPCHK(c, launch_spmv(in, EPI_PREC, w, nullptr, bj_op(s.M), v0, s.part[0], s.part[1], stop, col, c->stream));
        cnt = spmv_grid(in);
    } else {
        { Prof pf(c, "spmv", col, b_csr + 2 * n8);
          HIPCHK(c, launch_spmv(lsv_in(spmv_in(A, &A->tiles, v), A), EPI_PLAIN, s.tmp, nullptr, BjOp{}, nullptr, nullptr, nullptr, stop, col, c->stream)); }
        Prof pf(c, prec_cls(s.M), col, b_inv + 3 * n8);
        TRY(prec_apply(c, s.M, s.n, s.tmp, w, v0, s.part[0], s.part[1], s.G, stop, col, nullptr));
        cnt = s.G;
    }
    if (!want_dots) return VTK_OK;
    TRY(reduce(c, s.part[0], cnt, h0));
    return reduce(c, s.part[1], cnt, d0);
}

// step 0 of a band cycle through the x-line ring (x = v_0; the j = 0 dots only); across ranks the
// two halo lines first (12.8 KB at C3)
// band_nd: the same operator expression as the band steps, no read of D (the guard at the band
// step's launch holds here too: cyc_ring_ok asked bj8_tri(M))
int step_ring_start(Solver &s, const StepPlan &P, int j, const double *pj, double b_step, int &cnt) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    TRY(halo_exchange(A, pj));
    Prof pf(c, "spmv_bj_dc", j, b_step - (P.band_nd ? P.n8 : 0.0));
    SOFT(launch_lsv_ring_epi(P.band_nd ? EPI_PREC_DC_ND : EPI_PREC_DC, A->d_lsv, pj, nullptr, s.M->d_tri + s.M->tri_ld, s.w, nullptr,
                             nullptr, s.dcpart, s.n, (int)A->band_L, c->tune.cyc_ring, s.stop, j, &cnt,
                             c->stream, A->band_ghost ? A->d_halo : nullptr, A->band_lblk, A->band_xord));
    return VTK_OK;
}

// fused step across ranks: interior tiles while the halo is in flight, boundary tiles once it has
// landed; their partials side by side (cnt = both grids)
int step_fused_split(Solver &s, int j, const double *pj, double b_step, int &cnt) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    SpmvIn in = split_in(A, s.M, pj, true), bd = split_in(A, s.M, pj, false);
    in.halo = nullptr;   // interior tiles read owned columns only
    const double f_in = (A->use_sell ? A->g_in.count * 256.0 : (double)s.M->tiles_in.nrows) / std::max<double>(1.0, (double)s.n);
    // a rank with no x-neighbour data to send or receive (one rank) skips the exchange
    // and its event hand-offs; one without boundary rows skips the boundary launch
    const bool exch = A->n_send > 0 || A->n_halo > 0 || c->host_comm;
    const bool has_bd = A->use_sell ? A->g_bd.count > 0 : s.M->tiles_bd.ntiles > 0;
    if (exch) TRY(halo_exchange_async(A, pj));
    { Prof pf(c, "spmv_bj_dc", j, b_step * std::min(1.0, f_in));
      SOFT(launch_spmv_dc(in, s.w, bj_op(s.M), s.V, s.ld, j, s.dcpart, s.stop, j, c->stream)); }
    // the all-reduce below stays behind this rank's exchange on every rank (one order
    // of RCCL operations on the communicator)
    if (exch) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    cnt = spmv_grid(in);
    if (has_bd) {
        Prof pf(c, "spmv_bj_dc_bd", j, b_step * std::max(0.0, 1.0 - f_in));
        SOFT(launch_spmv_dc(bd, s.w, bj_op(s.M), s.V, s.ld, j, s.dcpart + spmv_grid(in), s.stop, j, c->stream));
        cnt += spmv_grid(bd);
    }
    return VTK_OK;
}

int step_fused(Solver &s, const StepPlan &P, int j, const double *pj, double b_step, int &cnt) {
    TRY(halo_exchange(s.A, pj));
    Prof pf(s.c, "spmv_bj_dc", j, b_step);
    const SpmvIn in = lsv_in(spmv_in(s.A, P.ft, pj), s.A);
    SOFT(launch_spmv_dc(in, s.w, bj_op(s.M), s.V, s.ld, j, s.dcpart, s.stop, j, s.c->stream));
    cnt = spmv_grid(in);
    return VTK_OK;
}

// line path (line Jacobi, the line product, the cyclic lines): the SpMV in one of its forms, then the
// kind's launches (kind_apply), each under its own class; the step's dots behind the last sweep where
// the kind has that form (the product: tuning line2_dc), else in reduce_step's launch_dc_dots (cnt 0)
int step_line(Solver &s, const StepPlan &P, int j, const double *pj, int &cnt) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    const int64_t n = s.n;
    const double n8 = P.n8;
    const int *stop = s.stop;
    TRY(halo_exchange(A, pj));
    if (P.line_fuse) {
        Prof pf(c, "line_dc", j, P.b_inv + 8.0 * (double)n + n8 * (j + 2));   // m, D, p, w, V_j
        SOFT(launch_line_spmv_dc(s.M->line, A->d_lsv, pj, s.w, s.V, s.ld, j, s.dcpart, s.G, stop, j, c->stream));
        cnt = s.G;
        return VTK_OK;
    }
    if (P.line_lsv) {
        // line-separable values: 12 B of matrix per row (codes + diagonal)
        Prof pf(c, "spmv_lsv", j, (P.line_canon ? 8.0 * (double)n : P.b_lsv) + 2 * n8);
        SOFT(launch_lsv_spmv(A->sell.d_pk, A->sell.d_dict, A->d_lsv, pj, c->dist ? A->d_halo : nullptr,
                             s.tmp, n, (int)A->band_L, A->band_ghost ? A->band_lblk : -1, stop, j,
                             c->stream, P.line_canon ? 1 : 0, 8192, c->tune.lsv_ring, A->band_ghost ? A->band_xord : 0));
    } else {
        Prof pf(c, "spmv", j, P.b_csr + 2 * n8);
        SOFT(launch_spmv(spmv_in(A, &A->tiles, pj), EPI_PLAIN, s.tmp, nullptr, BjOp{}, nullptr, nullptr, nullptr, stop, j, c->stream));
    }
    const StepDots dots{s.V, s.ld, j, s.dcpart};
    Apply a{s.tmp, s.w};
    a.grid = s.G, a.stop = stop, a.col = j, a.vote = &s.vote, a.prof = true;
    if (!s.cb && (P.line_dc || (P.line2_step && c->tune.line2_dc))) a.dots = &dots;
    return kind_apply(c, s.M, n, a, &cnt);
}

// 4D ring step.  Step 0's dots (|p|^2, p.w, |w|^2) in the same sweep; the later steps' dots in
// k_dc_dots (fused into the ring they cost 215.6 vs 201.5 ms per C4 solve: the ring then runs at
// 3 waves/SIMD and its basis reads wait behind the ring's)
int step_g4_ring(Solver &s, const StepPlan &P, int j, const double *pj, int &cnt) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    G4Dots dd;   // mode 2
    dd.part = s.dcpart;
    const G4Dots *dots = j == 0 ? &dd : nullptr;
    const char *cls = dots ? "spmv_bj_dc" : "spmv_bj";
    const double b_ring = P.b_solver + P.b_inv + 2 * P.n8;   // D, m, x, w
    const double *halo = A->g4.lblk >= 0 ? A->d_halo : nullptr;
    if (halo && P.split)   // a rank with nothing to exchange skips the exchange; a failed launch is voted
        return g4_ring_split(A, s.M, pj, s.w, A->n_send > 0 || A->n_halo > 0 || c->host_comm, &s.vote, cls, b_ring, dots, s.stop, j, &cnt);
    TRY(halo_exchange(A, pj));
    Prof pf(c, cls, j, b_ring);
    int grid = 0;
    SOFT(launch_g4_ring(A->g4, pj, halo, s.M->d_tri + s.M->tri_ld, s.w, s.n, A->fp32, c->tune.g4_ring, c->tune.g4_gr,
                        dots, &grid, s.stop, j, c->stream, 0, -1, 0, c->tune.g4_fast));
    if (dots) cnt = grid;
    return VTK_OK;
}

// the Neumann wrapper: w = N^-1 (A p_j).  The SpMV in the solver's form (tables / grid rows where the
// operator has them), then the wrapper's apply; cnt: the dots partials its last correction wrote
int step_neumann(Solver &s, const StepPlan &P, int j, const double *pj, int &cnt) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    TRY(halo_exchange(A, pj));
    { Prof pf(c, "spmv", j, P.b_solver + 2 * P.n8);
      SOFT(launch_spmv(lsv_in(spmv_in(A, &A->tiles, pj), A), EPI_PLAIN, s.tmp, nullptr, BjOp{}, nullptr, nullptr, nullptr, s.stop, j, c->stream)); }
    const StepDots dots{s.V, s.ld, j, s.dcpart};
    return prec_apply(c, s.M, s.n, s.tmp, s.w, nullptr, nullptr, nullptr, s.G, s.stop, j, &s.vote, s.cb ? nullptr : &dots, &cnt);
}

// the form step j takes (the plan's order of precedence)
int operator_step(Solver &s, const StepPlan &P, int j, double *pj, int &cnt) {
    const double b_step = P.b_solver + P.b_inv + P.n8 * (j + 2);   // matrix, BJ, p, w, V_j
    if (s.band && j > 0) {   // band: step j's w and partials come from the band step j-1
        cnt = s.band_grid(j - 1, P.band_opt);
        return VTK_OK;
    }
    if (P.ring0 && j == 0) return step_ring_start(s, P, j, pj, b_step, cnt);
    if (P.fused && P.split) return step_fused_split(s, j, pj, b_step, cnt);
    if (P.fused) return step_fused(s, P, j, pj, b_step, cnt);
    if (P.line_dc || P.line2_step || P.linec_step) return step_line(s, P, j, pj, cnt);
    if (P.ring4) return step_g4_ring(s, P, j, pj, cnt);
    if (P.neumann_step) return step_neumann(s, P, j, pj, cnt);
    Red h0, d0;
    return precond_matvec(s, P, pj, s.w, j, h0, d0, false);
}

// ---- the other pieces of a DCGS2 step ------------------------------------------------------------

// dots (unless the SpMV wrote them: cnt partials), all-reduce across ranks, scalar step
// (folding the finalize into the boundary launch's last workgroup was measured slower: one
// workgroup summing 2j+3 x ~1000 partials took as long as the 2j+3-workgroup launch)
// ev_ar (distributed): recorded on the main stream right after the all-reduce, so a
// communication the caller then issues on the comm stream starts only once the all-reduce
// has finished: every RCCL operation of the communicator runs in one order, on every rank
int reduce_step(Solver &s, int j, const double *w, int tag, int cnt, hipEvent_t ev_ar = nullptr) {
    vtk_ctx *c = s.c;
    if (cnt == 0 && s.cb) {
        Prof pf(c, "cb_dots", tag, (double)s.n * (4.0 * j + (w ? 16.0 : 8.0)));
        SOFT(launch_cb_dots(s.Vc, s.ld, j, s.cand(j), w, s.n, s.dcpart, s.G, s.stop, tag, c->stream));
        cnt = s.G;
    } else if (cnt == 0) {
        Prof pf(c, "dc_dots", tag, 8.0 * s.n * (j + (w ? 2 : 1)));
        SOFT(launch_dc_dots(s.V, s.ld, j, w, s.n, s.dcpart, s.G, s.stop, tag, c->stream));
        cnt = s.G;
    }
    const double *part = s.dcpart;
    if (c->dist) {
        { Prof pf(c, "dc_finalize", tag, 0.0);
          HIPCHK(c, launch_dc_finalize(s.dcpart, cnt, j, w != nullptr, c->d_scal, s.stop, tag, c->stream)); }
        {
            Prof pf(c, "allreduce", tag, 8.0 * DC_NQV);
            TRY(comm_allreduce(c, c->d_scal, DC_NQV));   // the dots + the failure vote
        }
        if (ev_ar) HIPCHK(c, hipEventRecord(ev_ar, c->stream));
        part = nullptr;
    }
    Prof pf(c, "dc_scalar", tag, 0.0);
    HIPCHK(c, launch_dc_scalar(part, cnt, c->d_scal, j, s.m, w == nullptr, s.Hraw, s.H, s.S, s.giv, s.cf, c->d_state, c->d_stop, c->stream, s.cb ? 1 : 0));
    return VTK_OK;
}

// distributed band step: the x-neighbours' edge lines of v_{j-1} and w_j travel to the ghost
// buffers on the comm stream once this step's all-reduce has finished (ev_pack, recorded by
// reduce_step across ranks: the RCCL operations never overlap; the exchange overlaps the scalar
// step); the band step waits for them
int ghost_exchange(Solver &s, int j, const double *w_cur) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    const int L = (int)A->band_L;
    if (!c->dist) HIPCHK(c, hipEventRecord(c->ev_pack, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_pack, 0));
    SOFT(launch_ghost_pack(s.V, s.ld, j, w_cur, s.n, L, s.gsend, A->band_off_first, A->band_off_last, c->comm_stream));
    TRY(comm_alltoallv(c, s.gsend, A->band_scnt, A->band_soff, s.grecv, A->band_rcnt, A->band_roff, ncclDouble, sizeof(double), c->comm_stream));
    SOFT(launch_ghost_unpack(s.grecv, A->band_off_left, A->band_off_right, j, s.m, L, s.ghost, c->comm_stream));
    HIPCHK(c, hipEventRecord(c->ev_halo, c->comm_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    return VTK_OK;
}

// band step: update pass of step j + SpMV, BJ and dots of step j+1 in one sweep over the x-lines
// reads V_k (k < j), w_{j-1} (v_0 at j = 0), w_j; writes v_j (j >= 1), w_{j+1} and, at
// j = m - 2 only, p_{j+1} (k_dc_update's operand)
// (VTK_PROF_PERJ=1: one profile class per step index, "band_step_jNN")
int band_step(Solver &s, const StepPlan &P, int j) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    const int m = s.m;
    const bool perj = c->tune.prof_perj != 0;
    Prof pf(c, perj && j < 20 ? P.jname[j] : "band_step", j, P.b_band + P.b_inv + P.n8 * (j + (j >= 1 ? 4 : 3) + (j == m - 2 ? 1 : 0)));
    BandK a;
    a.pk = A->sell.d_pk, a.dict = A->sell.d_dict, a.val = static_cast<const double *>(A->sell.d_val);
    a.mtri = s.M->d_tri + s.M->tri_ld;
    a.V = s.V, a.ld = s.ld, a.j = j, a.m = m;
    a.w_in = s.wbuf(j), a.w_prev = s.wbuf(j + 2), a.w_out = s.wbuf(j + 1);
    a.cf = s.cf, a.st = c->d_state, a.x = s.x, a.H = s.H, a.S = s.S, a.part = s.dcpart;
    a.n = s.n, a.L = (int)A->band_L, a.X = (int)(s.n / A->band_L), a.H_parts = s.band_H;
    a.ghost = s.ghost, a.left_blk = A->band_lblk, a.xord = A->band_xord;
    a.lsv = P.band_lsv ? A->d_lsv : nullptr;
    a.canon = P.band_lsv && A->lsv_canon && P.band_canon;
    // BAND_ND computes w = p + M^-1 (A - M) p, which is M^-1 A p only while a.mtri holds the
    // factors of A's CURRENT diagonal blocks.  band_eligible requires bj8_tri(M), which is false
    // unless M->epoch == A->values_epoch (a lagged M takes the non-band path).  A change that
    // lets a lagged M reach this launch must clear BAND_ND here, or the operator is wrong
    a.opt = P.band_opt;
    SOFT(launch_band_step(a, s.band_grid(j, a.opt), A->sell.uniform_w, c->stream));
    return VTK_OK;
}

// throttle: an event every ev_every steps (each record costs the stream a few us); the host
// waits for the event LOOKAHEAD or more steps back and acts on a stop the device has passed
// there.  Column cc stops in step cc (early commit) or cc+1: act only once every rank ran it.
// an event every 4 steps: r05 library A/B (profiles/r05_ev_every_ab.json) C3/8 slab +2 %,
// C3 +0.6 %; a stop is acted on at most 3 steps later (early-exit launches, ~us each)
int throttle(Solver &s, int j, bool &broke) {
    constexpr int ev_every = 4, R = LOOKAHEAD + 1;
    if ((j + 1) % ev_every == 0) {
        HIPCHK(s.c, hipEventRecord(s.ev[s.nev % R], s.c->stream));
        s.ev_step[s.nev++ % R] = j;
    }
    while (s.synced < s.nev && s.ev_step[s.synced % R] <= j - LOOKAHEAD) {
        const int js = s.ev_step[s.synced % R];
        HIPCHK(s.c, hipEventSynchronize(s.ev[s.synced++ % R]));
        if (*s.mirror <= js - 1) { broke = true; break; }
    }
    return VTK_OK;
}

// One restart cycle with DCGS2 (see vtk_kernels.hip, DCGS2 Arnoldi).  Step j's SpMV, dots,
// finalize and scalar kernels are tagged with column j-1 (the column they finalise), its update
// pass with column j: every kernel of step j returns at entry once stop_col < j.  After column
// m-1, a closing reduction finalises it.
int dcgs2_cycle(Solver &s, const StepPlan &P) {
    vtk_ctx *c = s.c;
    const int m = s.m;
    bool broke = false;
    s.nev = s.synced = 0;
    for (int j = 0; j < m && !broke; ++j) {
        double *pj = s.cand(j);
        double *w_cur = s.band ? s.wbuf(j) : s.w;
        int cnt = 0;
        TRY(operator_step(s, P, j, pj, cnt));
        const bool ghost_x = s.band && s.ghost && j <= m - 2;
        if (s.fail_pending && j == c->tune.fail_step) {   // test hook: as if this step's launch failed
            s.fail_pending = false;
            TRY(s.vote.launch(hipErrorLaunchFailure, "injected failure (tuning fail_step)"));
        }
        TRY(reduce_step(s, j, w_cur, j, cnt, ghost_x && c->dist ? c->ev_pack : nullptr));
        if (ghost_x) TRY(ghost_exchange(s, j, w_cur));
        if (s.band && j <= m - 2) {
            TRY(band_step(s, P, j));
        } else if (s.cb) {   // p_j, w, the j stored columns; v^_j and p_{j+1} written
            Prof pf(c, "cb_update", j, (double)s.n * (4.0 * j + 28.0));
            SOFT(launch_cb_update(s.Vc, s.ld, j, pj, w_cur, s.cand(j + 1), s.n, s.cf, s.G, c->d_state, s.x, s.H, s.S, m, c->stream));
        } else {
            Prof pf(c, "dc_update", j, P.n8 * (j + 4));
            SOFT(launch_dc_update(s.V, s.ld, j, w_cur, s.n, s.cf, s.G, c->d_state, s.x, s.H, s.S, m, P.fused ? 0 : 1, c->stream));
        }
        TRY(throttle(s, j, broke));
    }
    if (!broke) TRY(reduce_step(s, m, nullptr, m, 0));   // closing: only if column m-1 is still open
    return VTK_OK;
}

// One restart cycle with SciPy's modified Gram-Schmidt sequence (iterative.py:755-759)
int mgs_cycle(Solver &s, const StepPlan &P) {
    vtk_ctx *c = s.c;
    const int m = s.m;
    const int64_t n = s.n;
    const double n8 = P.n8;
    for (int col = 0; col < m; ++col) {
        double *vcol = s.V + (size_t)col * s.ld;
        Red h0, d0;
        TRY(precond_matvec(s, P, vcol, s.w, col, h0, d0));
        Red cur = d0;
        for (int k = 0; k <= col; ++k) {
            double *po = s.part[2 + (k & 1)];
            const double *vn = k < col ? s.V + (size_t)(k + 1) * s.ld : nullptr;
            { Prof pf(c, "mgs", col, (vn ? 4 : 3) * n8);
              SOFT(launch_mgs(cur, s.H + (size_t)col * (m + 1) + k, s.w, s.V + (size_t)k * s.ld, vn, n, po, s.G, s.stop, col, c->stream)); }
            TRY(reduce(c, po, s.G, cur));
        }
        { Prof pf(c, "tail", col, 2 * n8);
          SOFT(launch_tail(h0, cur, s.w, s.V + (size_t)(col + 1) * s.ld, n, col, m, s.H, s.S, s.giv, c->d_state, c->d_stop, s.G, c->stream)); }
        HIPCHK(c, hipEventRecord(s.ev[col % (LOOKAHEAD + 1)], c->stream));
        if (col >= LOOKAHEAD) {
            HIPCHK(c, hipEventSynchronize(s.ev[(col - LOOKAHEAD) % (LOOKAHEAD + 1)]));
            // Act only on a stop at a column whose tail every rank has completed (it is
            // behind the event just synchronised): a later column's flag may already be
            // visible on one rank and not on another, and the ranks must enqueue the same
            // sequence of collectives.
            if (*s.mirror <= col - LOOKAHEAD) break;
        }
    }
    return VTK_OK;
}

// r = b - A x, ||r|| into the state record; fused forms: also M^-1 r into V[0] with its partials
// (rz).  The plan chose the kernel; one tail pads (a no-op for the SpMV launches: across ranks
// their grids are GMAX, grid_for), reduces and finalises.
int residual(Solver &s, const StepPlan &P, Red &rz) {
    vtk_ctx *c = s.c;
    vtk_csr *A = s.A;
    vtk_prec *M = s.M;
    const int64_t n = s.n;
    const double *x = s.x, *b = s.b;
    double *prr = c->d_part + 4 * GMAX, *prz = P.resid_fused ? c->d_part + 5 * GMAX : nullptr;
    TRY(halo_exchange(A, x));
    Red rr;
    {
        Prof pf(c, P.resid_fused ? "spmv_resid_bj" : "spmv_resid", -1,
                P.resid_fused ? P.b_solver + prec_row_bytes(M) * n + 3 * P.n8 : P.b_solver + 3 * P.n8);
        int g = 0;
        if (P.resid_g4) {
            G4Dots dd;
            dd.mode = 3, dd.b = b, dd.p0 = prr, dd.p1 = prz;
            SOFT(launch_g4_ring(A->g4, x, A->g4.lblk >= 0 ? A->d_halo : nullptr, M->d_tri + M->tri_ld, s.start(), n, A->fp32,
                                c->tune.g4_ring, c->tune.g4_gr, &dd, &g, nullptr, 0, c->stream, 0, -1, 0, c->tune.g4_fast));
        } else if (P.resid_ring) {
            SOFT(launch_lsv_ring_epi(P.resid_fused ? EPI_RESID_PREC : EPI_RESID, A->d_lsv, x, b,
                                     P.resid_fused ? M->d_tri + M->tri_ld : nullptr, P.resid_fused ? s.start() : s.r, prr, prz,
                                     nullptr, n, (int)A->band_L, c->tune.cyc_ring, nullptr, 0, &g, c->stream,
                                     A->band_ghost ? A->d_halo : nullptr, A->band_lblk, A->band_xord));
        } else if (P.resid_fused) {
            const SpmvIn in = lsv_in(spmv_in(A, P.rtiles, x), A);
            SOFT(launch_spmv(in, EPI_RESID_PREC, s.start(), b, bj_op(M), nullptr, prr, prz, nullptr, 0, c->stream));
            g = spmv_grid(in);
        } else {
            const SpmvIn in = lsv_in(spmv_in(A, &A->tiles, x), A);
            SOFT(launch_spmv(in, EPI_RESID, s.r, b, BjOp{}, nullptr, prr, nullptr, nullptr, 0, c->stream));
            g = spmv_grid(in);
        }
        TRY(pad_partials(c, prr, prz, g));
        TRY(reduce(c, prr, g, rr));
        if (prz) TRY(reduce(c, prz, g, rz));
    }
    HIPCHK(c, launch_finalize(rr, &c->d_state->rnorm, 1, c->stream));
    return VTK_OK;
}

// ---- run_gmres's pieces ---------------------------------------------------------------------------

// a buffer the context keeps between solves, grown to `need` bytes (its contents dropped)
template <typename T>
int grow(vtk_ctx *c, T *&p, size_t &bytes, size_t need) {
    if (bytes >= need) return VTK_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    HIPCHK(c, hipMalloc(reinterpret_cast<void **>(&p), need));
    bytes = need;
    return VTK_OK;
}

// workspace: V[(m+1) x ld] (compressed basis: Vc[(m+1) x ld] floats | p_even | p_odd) | w | tmp | r | H[m x (m+1)] | S[m+1] | giv[2m]  (doubles), then the
// DCGS2 pieces, then (band) the third w buffer, the ghost lines [2][m+2][L] and the send / receive
// pieces
int layout_workspace(Solver &s) {
    vtk_ctx *c = s.c;
    const vtk_csr *A = s.A;
    const int m = s.m;
    const size_t ndc = s.dc ? (size_t)(m + 1) * (m + 1) + sizeof(DcCoef) / 8 + 8 + (size_t)DC_NQ * GMAX : 0;
    const size_t nghost = (s.band && A->band_ghost)
                              ? (size_t)2 * (m + 2) * A->band_L + 4 * (size_t)BAND_GHOST_VECS * A->band_L : 0;
    const size_t nedge = s.band ? (size_t)s.ld + nghost : 0;
    // the basis: (m + 1) ld doubles, or (compressed) (m + 1) ld floats and the two candidate vectors
    const size_t nbasis = s.cb ? (size_t)(m + 1) * s.ld / 2 + 2 * (size_t)s.ld : (size_t)(m + 1) * s.ld;
    const size_t nd = nbasis + 3 * (size_t)s.ld + (size_t)m * (m + 1) + (m + 1) + 2 * m + 64 + ndc + nedge + 16;
    TRY(grow(c, c->ws, c->ws_bytes, nd * sizeof(double)));
    double *wp = static_cast<double *>(c->ws);
    if (s.cb) {   // (ld is a multiple of 64: every column and both candidates stay 64-B aligned)
        s.Vc = reinterpret_cast<float *>(wp); wp += (size_t)(m + 1) * s.ld / 2;
        s.pc[0] = wp; wp += s.ld;
        s.pc[1] = wp; wp += s.ld;
    } else {
        s.V = wp; wp += (size_t)(m + 1) * s.ld;
    }
    c->basis_info = vtk_basis_info{c->basis, s.cb ? VTK_BASIS_F32 : VTK_BASIS_F64, (int64_t)(nbasis * sizeof(double)),
                                   (int64_t)(nd * sizeof(double))};
    s.w = wp; wp += s.ld;
    s.tmp = wp; wp += s.ld;
    s.r = wp; wp += s.ld;
    s.H = wp; wp += (size_t)m * (m + 1);
    s.S = wp; wp += m + 1;
    s.giv = wp; wp += 2 * m;
    if (s.dc) {
        wp = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(wp) + 63) & ~(uintptr_t)63);
        s.dcpart = wp; wp += (size_t)DC_NQ * GMAX;
        s.Hraw = wp; wp += (size_t)(m + 1) * (m + 1);
        s.cf = reinterpret_cast<DcCoef *>(wp);
        wp += sizeof(DcCoef) / 8 + 8;
        HIPCHK(c, hipMemsetAsync(s.Hraw, 0, (size_t)(m + 1) * (m + 1) * sizeof(double), c->stream));
    }
    if (s.band) {
        wp = reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(wp) + 63) & ~(uintptr_t)63);
        s.w3 = wp;
        if (A->band_ghost) {
            s.ghost = wp + s.ld;
            s.gsend = s.ghost + (size_t)2 * (m + 2) * A->band_L;
            s.grecv = s.gsend + 2 * (size_t)BAND_GHOST_VECS * A->band_L;
        }
    }
    HIPCHK(c, hipMemsetAsync(s.H, 0, (size_t)m * (m + 1) * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(s.giv, 0, (size_t)2 * m * sizeof(double), c->stream));
    return VTK_OK;
}

// capture of one restart cycle (vtk_gmres_capture, a test hook): the buffer once per solve; a
// solve that runs unarmed drops what an earlier one captured
struct Capture {
    bool on = false;
    size_t hsg = 0, hraw = 0;
    double *x = nullptr, *V = nullptr, *H = nullptr, *Hraw = nullptr, *cf = nullptr;
    int alloc(const Solver &s) {
        vtk_ctx *c = s.c;
        const int m = s.m;
        on = c->cap_cycle != -1;
        c->cap_valid = false;
        hsg = (size_t)m * (m + 1) + (m + 1) + 2 * m, hraw = (size_t)(m + 1) * (m + 1);
        if (!on) return VTK_OK;
        const size_t need = ((size_t)(m + 2) * s.ld + hsg + hraw + sizeof(DcCoef) / 8 + 8) * sizeof(double);
        TRY(grow(c, c->cap, c->cap_bytes, need));
        x = c->cap, V = x + s.ld, H = V + (size_t)(m + 1) * s.ld, Hraw = H + hsg, cf = Hraw + hraw;
        return VTK_OK;
    }
    // after the x update, before residual() writes the next v0 direction into V[0]
    int copy_cycle(const Solver &s) const {
        vtk_ctx *c = s.c;
        if (s.cb) HIPCHK(c, launch_cb_capture(s.Vc, s.ld, s.m, s.pc[0], s.pc[1], c->d_state, V, c->stream));
        else HIPCHK(c, hipMemcpyAsync(V, s.V, (size_t)(s.m + 1) * s.ld * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(H, s.H, hsg * sizeof(double), hipMemcpyDeviceToDevice, c->stream));   // H | S | giv
        if (s.dc) {
            HIPCHK(c, hipMemcpyAsync(Hraw, s.Hraw, hraw * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(cf, s.cf, sizeof(DcCoef), hipMemcpyDeviceToDevice, c->stream));
        }
        return VTK_OK;
    }
    // the columns of V that are final at cycle end (the rule: include/vtkrylov.h)
    void commit(const Solver &s, const GmresState *hs, int64_t it, int last) const {
        vtk_ctx *c = s.c;
        const int fin = s.dc ? (hs->xup_tag >= 0 ? std::max(hs->xup_tag, 1) : s.m) : last + 1 + (hs->breakdown ? 0 : 1);
        c->cap_info = vtk_arnoldi_info{s.n, s.ld, s.m, (int)it, last + 1, fin, s.dc ? VTK_ORTH_DCGS2 : VTK_ORTH_MGS,
                                       s.band ? 1 : 0, s.dc ? 1 : 0, hs->stop_col, hs->breakdown, hs->xup_tag};
        c->cap_valid = true;
    }
};

// the cycle's profile records once its stop column is known: the x update's bytes, and which
// launch ran it
void cycle_profile(const Solver &s, const GmresState *hs, size_t xup_idx, int last) {
    vtk_ctx *c = s.c;
    const double n8 = 8.0 * s.n;
    // V[0..last] (or V_last and p_last), x in/out; compressed: 4 B per stored entry
    const double xb = (s.cb ? 0.5 : 1.0) * n8 * (last + 1) + 2 * n8;
    if (xup_idx < c->prof_pending.size()) c->prof_pending[xup_idx].bytes = xb;
    if (hs->xup_tag >= 0) {
        // the x update ran in update pass xup_tag: account it as the "xupdate" class and
        // drop the host-enqueued k_xupdate (it returned at entry)
        const int cu = prof_class(c, s.cb ? "cb_update" : "dc_update"), cb = prof_class(c, "band_step"),
                  cx = prof_class(c, s.cb ? "cb_xupdate" : "xupdate");
        for (size_t i = 0; i < xup_idx && i < c->prof_pending.size(); ++i) {
            auto &p = c->prof_pending[i];
            if ((p.cls == cu || p.cls == cb) && p.col == hs->xup_tag) { p.cls = cx; p.col = -1; p.bytes = xb; }
        }
        if (xup_idx < c->prof_pending.size()) c->prof_pending[xup_idx].col = BIG_COL;
    }
    prof_flush(c, last);
}

// ||b||, ||M b|| (M b into V[0]) and x.any(); then the state record on the host (hs)
int initial_norms(Solver &s, bool &r_is_b, bool &basis_mixed) {
    vtk_ctx *c = s.c;
    vtk_prec *M = s.M;
    const int64_t n = s.n;
    GmresState *ds = c->d_state;
    const double n8 = 8.0 * n;
    Red rb, rmb;
    // ||b|| and ||M b|| (iterative.py:708, :714)
    { Prof pf(c, "dot", -1, n8);
      HIPCHK(c, launch_dot(s.b, nullptr, n, s.part[0], s.G, c->stream)); }
    TRY(reduce(c, s.part[0], s.G, rb));
    HIPCHK(c, launch_finalize(rb, &ds->scal[0], 1, c->stream));
    // M b goes to V[0] (the cycle's start direction): with x0 = 0 it is the first cycle's psolve(r) (run_gmres)
    { Prof pf(c, prec_cls(M), -1, prec_row_bytes(M) * n + 2 * n8);
      TRY(prec_apply(c, M, n, s.b, s.start(), nullptr, s.part[1], nullptr, s.G, nullptr, 0, nullptr)); }
    TRY(reduce(c, s.part[1], s.G, rmb));
    HIPCHK(c, launch_finalize(rmb, &ds->scal[1], 1, c->stream));
    // `r = b - matvec(x) if x.any() else b.copy()` (iterative.py:737): any nonzero x0 on any rank
    HIPCHK(c, hipMemsetAsync(&ds->scal[2], 0, sizeof(double), c->stream));
    { Prof pf(c, "any", -1, n8);
      HIPCHK(c, launch_any_nonzero(s.x, n, &ds->scal[2], c->stream)); }
    // ... and, in the same all-reduce, the ranks' choice of basis storage: [3] the ranks that chose
    // float32, [4] the ranks (every rank joins whatever it chose; basis_mixed: they disagree)
    double flags[3] = {0.0, 0.0, 0.0};
    if (c->dist) {
        const double mine[2] = {c->basis == VTK_BASIS_F32 ? 1.0 : 0.0, 1.0};
        HIPCHK(c, hipMemcpyAsync(&ds->scal[3], mine, sizeof(mine), hipMemcpyHostToDevice, c->stream));
        TRY(comm_allreduce(c, &ds->scal[2], 3));
    }
    HIPCHK(c, hipMemcpyAsync(flags, &ds->scal[2], (c->dist ? 3 : 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r_is_b = flags[0] == 0.0;
    basis_mixed = c->dist && flags[1] != 0.0 && flags[1] != flags[2];
    return VTK_OK;
}

// every rank takes the same path: the band step exchanges ghost lines with its neighbours each
// step, so one rank falling back alone would leave its peers' sends unmatched.  The agreement (an
// all-reduce and a host sync) is needed only when some rank could take the band (band_eligible)
int band_agree(Solver &s, bool possible) {
    vtk_ctx *c = s.c;
    if (!c->dist || !possible) return VTK_OK;
    double mine = s.band ? 0.0 : 1.0, off = 0.0;
    HIPCHK(c, hipMemcpyAsync(&c->d_scal[DC_NQ + 2], &mine, sizeof(double), hipMemcpyHostToDevice, c->stream));
    TRY(comm_allreduce(c, &c->d_scal[DC_NQ + 2], 1));
    TRY(read_back(c, off, &c->d_scal[DC_NQ + 2]));
    if (off != 0.0) s.band = false;
    return VTK_OK;
}

// One restart cycle: its start v0 = M^-1 r / ||M^-1 r||, S = [tmp, 0, ...] (iterative.py:742-748; r_ready: V[0] holds
// M^-1 r already, rz its partials), the Arnoldi steps, x += y @ V[:col+1] (:799-814), r = b - A x and rnorm (:816-817),
// the ranks' failure vote; then the state record on the host (hs) and the cycle's bookkeeping
int run_cycle(Solver &s, const StepPlan &P, const Capture &cap, int64_t it, bool r_ready, Red &rz, vtk_stats &st) {
    vtk_ctx *c = s.c;
    const int64_t n = s.n;
    const int m = s.m;
    GmresState *ds = c->d_state, *hs = c->h_state;
    HIPCHK(c, hipMemcpyAsync(&ds->ptol, &hs->ptol, sizeof(double), hipMemcpyHostToDevice, c->stream));
    Red rv = rz;
    if (!r_ready) {
        { Prof pf(c, prec_cls(s.M), -1, P.b_inv + 2 * P.n8);
          TRY(prec_apply(c, s.M, n, s.r, s.start(), nullptr, s.part[0], nullptr, s.G, nullptr, 0, &s.vote)); }
        TRY(reduce(c, s.part[0], s.G, rv));
    }
    if (s.cb) {   // the direction read, v^_0 stored and written back widened
        Prof pf(c, "cb_scale0", -1, 20.0 * n);
        SOFT(launch_cb_scale0(rv, s.pc[0], s.Vc, n, s.S, m, ds, s.G, c->stream));
    } else {
        Prof pf(c, "scale0", -1, 2 * P.n8);
        SOFT(launch_scale0(rv, s.V, n, s.S, m, ds, s.G, c->stream));
    }
    *s.mirror = BIG_COL;
    // x as the cycle finds it: the x update may run inside an update pass of the cycle
    const bool cap_now = cap.on && (c->cap_cycle == -2 || c->cap_cycle == it);
    if (cap_now) HIPCHK(c, hipMemcpyAsync(cap.x, s.x, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (s.dc) {
        HIPCHK(c, hipMemsetAsync(s.cf->committed, 0, sizeof(s.cf->committed), c->stream));
        TRY(dcgs2_cycle(s, P));
    } else {
        TRY(mgs_cycle(s, P));
    }
    const size_t xup_idx = c->prof_pending.size();
    if (s.cb) {
        Prof pf(c, "cb_xupdate", -1, 0.0);
        SOFT(launch_cb_xupdate(s.H, s.S, s.Vc, s.ld, s.x, n, m, ds, s.G, c->stream));
    } else {
        Prof pf(c, "xupdate", -1, 0.0);   // bytes set once the stop column is known
        SOFT(launch_xupdate(s.H, s.S, s.V, s.ld, s.x, n, m, ds, s.G, c->stream));
    }
    if (cap_now) TRY(cap.copy_cycle(s));
    TRY(residual(s, P, rz));
    // across ranks: the cycle's failure vote (a launch of some rank failed in this cycle; the
    // per-step vote has already stopped the Arnoldi steps at the same step on every rank)
    double vote = 0.0;
    if (c->dist) {
        TRY(comm_allreduce(c, &c->d_scal[DC_VOTE + 1], 1));
        HIPCHK(c, hipMemcpyAsync(&vote, &c->d_scal[DC_VOTE + 1], sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    TRY(read_back(c, *hs, ds));
    if (vote != 0.0) {
        prof_flush(c);
        if (s.vote.local_rc != VTK_OK) return s.vote.local_rc;
        return fail(c, VTK_ERR_PEER, "a peer rank failed in restart cycle " + std::to_string(it) +
                                         (hs->breakdown == PEER_FAILED ? " at Arnoldi step " + std::to_string(hs->stop_col + 1) : std::string()) +
                                         "; every rank left the solve there");
    }
    const int last = hs->stop_col < m ? hs->stop_col : m - 1;
    if (cap_now) cap.commit(s, hs, it, last);
    if (c->prof_on) cycle_profile(s, hs, xup_idx, last);
    const double bytes_spmv = P.b_csr + 16.0 * n, bytes_pc = P.b_inv + 16.0 * n;
    // per step: operator, preconditioner, the two basis passes (float64 8(j+4) + 8(j+2) B per row and
    // 16 B for the step's other vector traffic; compressed: 4j+28 + 4j+16); then the x update
    for (int j = 0; j <= last; ++j) st.bytes_moved += bytes_spmv + bytes_pc + (s.cb ? (double)n * (8.0 * j + 60.0) : 8.0 * n * (2 * j + 8));
    st.bytes_moved += bytes_spmv + 24.0 * n + bytes_pc + 24.0 * n + (s.cb ? (double)n * (4.0 * (last + 1) + 16.0) : 8.0 * n * (last + 2));
    st.restarts = it + 1;
    return VTK_OK;
}

}  // namespace

// ---- shared with vtk_precond_matvec (vtk_api.cpp) -----------------------------------------------

// grid rows with x staged through LDS (k_g4_ring; tuning g4_ring; BJ(8) tridiag)
// (only for grids whose window and tables fit the kernel's LDS, g4_ring_fits; larger 4D
// grids keep the SELL grid-row kernels)
bool vtk::g4_ring_ok(vtk_ctx *c, const vtk_csr *A, const vtk_prec *M) {
    return A->d_g4tab && c->tune.grid4 && c->tune.g4_ring > 0 && A->use_sell && bj8_tri(M) && g4_ring_fits(A->g4, A->n_local, c->tune.g4_gr);
}

// the SpMV inside the line sweep kernel (k_line_spmv_dc, tuning line_fuse): one rank, the table
// SpMV's conditions (line_lsv_ok), canonical rows, compact factors over the whole slab
bool vtk::line_fuse_ok(vtk_ctx *c, const vtk_csr *A, const vtk_prec *M) {
    if (!M || M->kind != VTK_PREC_LINE || !line_lsv_ok(c, A) || !A->lsv_canon || !c->tune.sell_canon || !c->tune.line_fuse || c->dist)
        return false;
    const LineOp &lo = M->line;
    const int64_t n = A->n_local;
    return lo.seg >= 1 && lo.seg <= 32 && lo.compact && lo.stride == A->band_L && lo.row0 == 0 && lo.n == n &&
           lo.j0 == 0 && lo.jn == lo.stride && lo.ac && lo.i_lo == 0 && lo.i_hi == n / lo.stride - 1 && n / lo.stride >= 3;
}

// The 4D ring step across ranks: the rows [S4, n - S4) read no halo plane -- their groups run while
// the exchange is in flight (comm stream), the first / last plane's groups after it lands.  Groups per
// workgroup: with dots no fewer than fit GMAX - 3 workgroups (g4_ring_per >= 1, so without dots it decides alone).
// The callers' differences, one parameter each.  exch: start the exchange and wait for it (the solver: not on a
// rank with nothing to exchange).  vote: a failed launch is voted (null: it returns at once).  cls: the interior
// launch's profile class, the boundary launches take "spmv_bj_bd", `bytes` split by rows (null: the caller brackets
// the whole call).  dots: step 0's partials, the three launches' side by side, *cnt of them
int vtk::g4_ring_split(vtk_csr *A, const vtk_prec *M, const double *x, double *w, bool exch, Vote *vote, const char *cls,
                       double bytes, const G4Dots *dots, const int *stop, int col, int *cnt) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local;
    const int G = g4_ring_group(c->tune.g4_gr);
    const int64_t S4 = (int64_t)A->g4.Ny * A->g4.Nvx * A->g4.Nvy, ng = (n + G - 1) / G;
    int64_t gi_lo = (S4 + G - 1) / G, gi_hi = (n - S4) / G;
    if (gi_hi <= gi_lo) gi_lo = gi_hi = 0;   // no interior group: all after the exchange
    const int per = (int)std::max<int64_t>(g4_ring_per(ng, S4, G, std::max(1, c->tune.g4_ring)), dots ? (ng + GMAX - 4) / (GMAX - 3) : 1);
    const double f_in = (double)(gi_hi - gi_lo) * G / std::max<double>(1.0, (double)n);
    G4Dots dd = dots ? *dots : G4Dots{};
    int g[3] = {0, 0, 0};
    auto launch = [&](int k, int64_t lo, int64_t hi) -> int {
        const hipError_t e = launch_g4_ring(A->g4, x, A->d_halo, M->d_tri + M->tri_ld, w, n, A->fp32, c->tune.g4_ring, c->tune.g4_gr,
                                            dots ? &dd : nullptr, &g[k], stop, col, c->stream, (int)lo, (int)hi, per, c->tune.g4_fast);
        return soft_launch(c, vote, e, "launch_g4_ring");
    };
    if (exch) TRY(halo_exchange_async(A, x));
    {
        Prof pf(c, cls, col, bytes * (double)(gi_hi - gi_lo) * G / std::max<double>(1.0, (double)n));
        if (gi_hi > gi_lo) TRY(launch(0, gi_lo, gi_hi));
    }
    if (exch) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_halo, 0));
    Prof pf(c, cls ? "spmv_bj_bd" : nullptr, col, bytes * std::max(0.0, 1.0 - f_in));
    dd.part_off = g[0];
    TRY(launch(1, 0, gi_hi > gi_lo ? gi_lo : ng));
    dd.part_off = g[0] + g[1];
    if (gi_hi > gi_lo) TRY(launch(2, gi_hi, ng));
    if (dots) *cnt = g[0] + g[1] + g[2];
    return VTK_OK;
}

int vtk::run_gmres(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
                   int restart, int64_t maxiter, int *info, vtk_stats *stout) {
    vtk_ctx *c = A->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = A->n_local, N = A->n_global;
    if (maxiter <= 0) maxiter = N * 10;                     // iterative.py:726-727
    if (restart <= 0) restart = 20;                         // :729-730
    if (restart > N) restart = (int)N;                      // :731
    if (restart > MAX_RESTART) return fail(c, VTK_ERR_ARG, "restart exceeds MAX_RESTART");
    if (restart < 1) return fail(c, VTK_ERR_ARG, "empty system");
    const int m = restart;
    Solver s{A, M, c, n, round_up(std::max<int64_t>(n, 1), 64), m, grid_for(c, vector_grid(n)), b, x};
    for (int k = 0; k < 4; ++k) s.part[k] = c->d_part + k * GMAX;
    s.vote = Vote{c, &c->d_scal[DC_VOTE + 1]};
    s.dc = c->orth == VTK_ORTH_DCGS2 || (c->orth == VTK_ORTH_AUTO && m <= DC_MAXJ);
    if (s.dc && m > DC_MAXJ) return fail(c, VTK_ERR_ARG, "DCGS2 supports restart <= 32 (use VTK_ORTH_MGS)");
    // the compressed basis runs on the DCGS2 sequence only.  One rank refuses here; across ranks after
    // the ranks have compared their choices (initial_norms), so that all of them leave together
    const bool cb_mgs = c->basis == VTK_BASIS_F32 && !s.dc;
    const char *cb_mgs_msg = "VTK_BASIS_F32 runs on the DCGS2 sequence only (restart <= 32 with VTK_ORTH_AUTO or VTK_ORTH_DCGS2); "
                             "the MGS sequence keeps the float64 basis";
    if (cb_mgs && !c->dist) return fail(c, VTK_ERR_ARG, cb_mgs_msg);
    s.cb = c->basis == VTK_BASIS_F32 && s.dc;
    bool band_possible = false;
    s.band = band_eligible(s, band_possible) && !s.cb;
    TRY(band_agree(s, band_possible));
    TRY(layout_workspace(s));
    Capture cap;
    TRY(cap.alloc(s));
    const StepPlan P = step_plan(s);
    GmresState *ds = c->d_state, *hs = c->h_state;
    std::memset(hs, 0, sizeof(GmresState));
    hs->stop_col = BIG_COL;
    hs->xup_tag = -1;
    HIPCHK(c, hipMemcpyAsync(ds, hs, sizeof(GmresState), hipMemcpyHostToDevice, c->stream));
    if (c->dist) HIPCHK(c, hipMemsetAsync(&c->d_scal[DC_VOTE + 1], 0, sizeof(double), c->stream));   // no failure yet
    s.fail_pending = c->tune.fail_step >= 0;
    bool r_is_b = true, basis_mixed = false;
    TRY(initial_norms(s, r_is_b, basis_mixed));
    if (basis_mixed) return fail(c, VTK_ERR_ARG, "vtk_gmres: the ranks disagree on the basis storage (vtk_gmres_set_basis): set the same on every rank");
    if (cb_mgs) return fail(c, VTK_ERR_ARG, cb_mgs_msg);
    Red rz{c->d_part + 5 * GMAX, spmv_grid(spmv_in(A, P.rtiles, x))};
    if (r_is_b) {
        // r = b: ||r|| = ||b||, and psolve(r) = M b is already in V[0] with its partials
        HIPCHK(c, hipMemcpyAsync(&ds->rnorm, &ds->scal[0], sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        rz = Red{s.part[1], s.G};
    } else {
        TRY(residual(s, P, rz));
    }
    TRY(read_back(c, *hs, ds));
    const double bnrm2 = hs->scal[0], Mb_nrm2 = hs->scal[1];
    const double eps = 2.220446049250313e-16;
    atol = std::max(atol, rtol * bnrm2);                    // _get_atol_rtol :19
    vtk_stats st{};
    st.bnorm = bnrm2;
    st.atol_eff = atol;
    st.orth = s.dc ? VTK_ORTH_DCGS2 : VTK_ORTH_MGS;
    st.band = s.band ? 1 : 0;
    if (bnrm2 == 0.0) {                                     // :712-713 -> x = b
        HIPCHK(c, hipMemcpyAsync(x, b, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return solve_done(info, 0, st, stout, t0);
    }
    double rnorm = st.rnorm = hs->rnorm;
    if (rnorm < atol) return solve_done(info, 0, st, stout, t0);   // :738-739
    double ptol_max_factor = 1.0;
    double ptol = Mb_nrm2 * std::min(ptol_max_factor, atol / bnrm2);   // :723
    double presid = 0.0;
    EvRing ev;
    TRY(ev.create(c));
    s.ev = ev.e;
    s.stop = &ds->stop_col;
    s.mirror = c->h_stop;
    bool brk = false;
    for (int64_t it = 0; it < maxiter; ++it) {
        hs->ptol = ptol;
        // the fused residual wrote M^-1 r into V[0]; so did initial_norms when r = b
        TRY(run_cycle(s, P, cap, it, P.resid_fused || (it == 0 && r_is_b), rz, st));
        rnorm = hs->rnorm;
        presid = hs->presid;
        brk = hs->breakdown != 0;
        if (rnorm <= atol) break;                                                   // :824
        else if (brk) break;                                                        // :826
        else if (presid <= ptol) ptol_max_factor = std::max(eps, 0.25 * ptol_max_factor);   // :830
        else ptol_max_factor = std::min(1.0, 1.5 * ptol_max_factor);              // :833
        ptol = presid * std::min(ptol_max_factor, atol / rnorm);                    // :835
    }
    prof_flush(c);
    st.inner_iters = hs->inner;
    st.presid = presid;
    st.rnorm = rnorm;
    st.breakdown = brk ? 1 : 0;
    return solve_done(info, rnorm <= atol ? 0 : (int)std::min<int64_t>(maxiter, INT32_MAX), st, stout, t0);   // :840
}
