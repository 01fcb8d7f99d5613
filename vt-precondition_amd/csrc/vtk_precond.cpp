// vtk_precond.cpp -- preconditioner factors from the operator's current values: block Jacobi, line
// Jacobi, the two-direction line product, the periodic whole lines (vtk_*_create and vtk_prec_refresh call these).
#include <climits>
#include <mutex>
#include <unordered_map>

#include "vtk_driver.hpp"

using namespace vtk;

namespace vtk {

// ---- preconditioner factors from the operator's current values ------------------------------
// What vtk_bjacobi_create_ex computes and vtk_prec_refresh repeats, into the storage M owns
// (d_inv; d_tri allocated here when the block size has tridiagonal factors and M has none).
// Every allocation precedes the first overwrite.  VTK_ERR_SINGULAR: a singular block.
int bj_factor(vtk_prec *M) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    const int bs = M->bs;
    DBuf sing, work, flags;
    TRY(dalloc(c, sing, sizeof(int)));
    const bool pow2 = (bs & (bs - 1)) == 0 && bs <= 32;
    if (!pow2) TRY(dalloc(c, work, std::max<int64_t>(M->nb, 1) * bs * bs * sizeof(double)));
    const bool tri = bs == 2 || bs == 4 || bs == 8;
    if (tri) {
        TRY(dalloc(c, flags, sizeof(int)));
        if (!M->d_tri) {
            M->tri_ld = std::max<int64_t>(M->nb, 1) * bs;
            HIPCHK(c, hipMalloc(&M->d_tri, 3 * M->tri_ld * sizeof(double)));
        }
    }
    const int init = INT32_MAX;
    HIPCHK(c, hipMemcpyAsync(sing.p, &init, sizeof(int), hipMemcpyHostToDevice, c->stream));
    {
        Prof pf(c, M->setup == VTK_BJ_SETUP_MFMA ? "bj_setup_mfma" : "bj_setup", -1,
                (double)M->nb * bs * bs * 8.0 + matrix_bytes(A));
        if (M->setup == VTK_BJ_SETUP_MFMA)
            HIPCHK(c, launch_bj_setup_mfma(A->d_indptr, A->d_indices, A->d_data, A->fp32, A->n_local, bs, M->d_inv,
                                           sing.as<int>(), c->stream));
        else
            HIPCHK(c, launch_bj_setup(A->d_indptr, A->d_indices, A->d_data, A->fp32, A->n_local, bs, M->d_inv,
                                      sing.as<int>(), work.as<double>(), c->stream));
    }
    prof_flush(c);
    int sb = 0;
    TRY(read_back(c, sb, sing.p));
    if (sb != INT32_MAX) return fail(c, VTK_ERR_SINGULAR, "vtk_bjacobi_create: singular diagonal block " + std::to_string(sb + A->row_begin / bs));
    M->tri_ok = false;
    if (tri) {
        // tridiagonal blocks (the v-direction coupling of the Vlasov operators): LU factors
        HIPCHK(c, hipMemsetAsync(flags.p, 0, sizeof(int), c->stream));
        { Prof pf(c, "bj_tri_setup", -1, (double)M->nb * bs * bs * 8.0 + 24.0 * (double)M->tri_ld + matrix_bytes(A));
          HIPCHK(c, launch_bj_tri_setup(A->d_indptr, A->d_indices, A->d_data, A->fp32, A->n_local, bs, M->d_inv, M->d_tri, M->tri_ld, flags.as<int>(), c->stream)); }
        if (c->prof_on) prof_flush(c);
        int fl = 0;
        TRY(read_back(c, fl, flags.p));
        M->tri_ok = fl == 0;
        if (!M->tri_ok) {
            (void)hipFree(M->d_tri);
            M->d_tri = nullptr;
        }
    }
    return VTK_OK;
}

// One line direction (line Jacobi, or either factor of the line product): Thomas factors into
// L.f, then the x-invariance check of the couplings; the compact tables are built in a
// scope-owned buffer and committed (or dropped) at the end.  compact_req / compact_ok: vtk_prec's
// (a vtk_linejacobi_set_compact(0) request is kept).  A zero or non-finite pivot: bad_row = the
// smallest such global row (else ~0), VTK_OK, and L.ac left as it was.
static int line_factor_op(vtk_csr *A, LineOp &L, int compact_req, bool &compact_ok, unsigned long long &bad_row) {
    vtk_ctx *c = A->ctx;
    DBuf bad, ext, acb;
    const int64_t jn = L.jn;
    TRY(dalloc(c, bad, sizeof(unsigned long long)));
    TRY(dalloc(c, ext, 4 * std::max<int64_t>(jn, 1) * sizeof(unsigned long long)));
    TRY(dalloc(c, acb, 2 * (size_t)std::max<int64_t>(jn, 1) * sizeof(double)));
    const unsigned long long none = ~0ull;
    std::vector<unsigned long long> hx(4 * (size_t)jn);
    for (int64_t j = 0; j < jn; ++j) {   // min | max | min | max
        hx[j] = none; hx[jn + j] = 0; hx[2 * jn + j] = none; hx[3 * jn + j] = 0;
    }
    HIPCHK(c, hipMemcpyAsync(bad.p, &none, sizeof(none), hipMemcpyHostToDevice, c->stream));
    if (jn) HIPCHK(c, hipMemcpyAsync(ext.p, hx.data(), hx.size() * 8, hipMemcpyHostToDevice, c->stream));
    { Prof pf(c, "line_setup", -1, 24.0 * (double)A->n_local + matrix_bytes(A));
      HIPCHK(c, launch_line_setup(A->d_indptr, A->d_indices, A->d_data, A->fp32, L, bad.as<unsigned long long>(), ext.as<unsigned long long>(), c->stream)); }
    if (c->prof_on) prof_flush(c);
    unsigned long long br = none;
    HIPCHK(c, hipMemcpyAsync(&br, bad.p, sizeof(br), hipMemcpyDeviceToHost, c->stream));
    if (jn) HIPCHK(c, hipMemcpyAsync(hx.data(), ext.p, hx.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bad_row = br;
    if (br != none) return VTK_OK;
    // x-invariant couplings (every line's a's bit-equal, likewise its c's): the apply forms l and
    // g from a_j, c_j and m (16 B/row read instead of 32); lines without any a (c) take 0
    bool inv = jn > 0;
    std::vector<double> ac(2 * (size_t)std::max<int64_t>(jn, 1), 0.0);
    for (int64_t j = 0; j < jn && inv; ++j) {
        for (int w = 0; w < 2; ++w) {
            const unsigned long long lo = hx[2 * w * jn + j], hi = hx[(2 * w + 1) * jn + j];
            if (lo > hi) continue;   // no row of this line has the coupling
            if (lo != hi) { inv = false; break; }
            std::memcpy(&ac[w * jn + j], &lo, 8);
        }
    }
    if (inv) HIPCHK(c, hipMemcpy(acb.p, ac.data(), ac.size() * sizeof(double), hipMemcpyHostToDevice));
    (void)hipFree(L.ac);
    L.ac = nullptr;
    L.compact = 0;
    if (inv) {
        L.ac = acb.as<double>();
        acb.p = nullptr;   // owned by the preconditioner now
        L.compact = compact_req == 0 ? 0 : 1;
    }
    compact_ok = inv;
    return VTK_OK;
}

// The same as bj_factor for line Jacobi (vtk_linejacobi_create / vtk_prec_refresh).
// VTK_ERR_SINGULAR: a zero or non-finite pivot.
int line_factor(vtk_prec *M) {
    unsigned long long br = ~0ull;
    TRY(line_factor_op(M->A, M->line, M->compact_req, M->line_compact_ok, br));
    if (br != ~0ull)
        return fail(M->A->ctx, VTK_ERR_SINGULAR, "vtk_linejacobi_create: zero or non-finite line pivot at row " + std::to_string(br));
    return VTK_OK;
}

// The line product (vtk_lineproduct_create / vtk_prec_refresh): both directions' factors and
// constant-coupling checks, and D = A's diagonal.  VTK_ERR_SINGULAR: a zero or non-finite pivot in
// either direction (the smaller row is reported).
int line2_factor(vtk_prec *M) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    unsigned long long br1 = ~0ull, br2 = ~0ull;
    TRY(line_factor_op(A, M->line, -1, M->line_compact_ok, br1));
    TRY(line_factor_op(A, M->line2, -1, M->line2_compact_ok, br2));
    { Prof pf(c, "line2_diag", -1, 8.0 * (double)A->n_local + matrix_bytes(A));
      HIPCHK(c, launch_line2_diag(A->d_indptr, A->d_indices, A->d_data, A->fp32, A->n_local, M->d_diag, c->stream)); }
    if (c->prof_on) prof_flush(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long br = std::min(br1, br2);
    if (br != ~0ull)
        return fail(c, VTK_ERR_SINGULAR, "vtk_lineproduct_create: zero or non-finite line pivot at row " + std::to_string(br));
    return VTK_OK;
}

// ---- periodic whole lines (vtk_linecyclic_create; vtk_linec.hip) ----------------
void linec_free(LineC &C) {
    for (int k = 0; k < LINEC_MAXLEV; ++k) {
        (void)hipFree(C.lev[k].f);
        (void)hipFree(C.lev[k].x);
        C.lev[k] = LineCLevel{};
    }
    (void)hipFree(C.minv);
    C.minv = nullptr;
    C.nlev = 0;
}

// The levels of M->linec and their storage (the arguments are checked by the caller).  Level 0 cuts
// the lines into segments of seg; a level of the separators is cut again while it has more than
// linec_serial unknowns per line and more than one segment; the last level is one segment per line.
int linec_plan(vtk_prec *M, int64_t stride, int64_t period, int64_t seg) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    LineC &C = M->linec;
    C.n = A->n_local;
    C.row0 = A->row_begin;
    C.stride = stride;
    C.period = period;
    C.seg = seg;
    C.nblk = A->n_local / (stride * period);
    C.serial = std::max(1, c->tune.linec_serial);
    const int64_t lines = C.nblk * stride;
    int64_t P = period;
    for (int k = 0;; ++k) {
        if (k >= LINEC_MAXLEV) return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create: too many levels");
        LineCLevel &v = C.lev[k];
        const bool last = k > 0 && (P <= C.serial || P <= seg);
        v.period = P;
        v.seg = last ? P : std::min(seg, P);
        v.nseg = (P + v.seg - 1) / v.seg;
        v.n = lines * P;
        HIPCHK(c, hipMalloc(&v.f, 5 * (size_t)std::max<int64_t>(v.n, 1) * sizeof(double)));
        if (k > 0) HIPCHK(c, hipMalloc(&v.x, (size_t)std::max<int64_t>(v.n, 1) * sizeof(double)));
        C.nlev = k + 1;
        if (last) break;
        P = v.nseg;
    }
    HIPCHK(c, hipMalloc(&C.minv, (size_t)std::max<int64_t>(lines, 1) * sizeof(double)));
    return VTK_OK;
}

// global row of element idx of level lev: a level's element i is the separator of segment i of the
// level below
static int64_t linec_row(const LineC &C, int lev, int64_t idx) {
    const int64_t j = idx % C.stride, t = idx / C.stride;
    int64_t i = t % C.lev[lev].period;
    const int64_t blk = t / C.lev[lev].period;
    for (int k = lev; k > 0; --k) i = std::min((i + 1) * C.lev[k - 1].seg, C.lev[k - 1].period) - 1;
    return C.row0 + (blk * C.period + i) * C.stride + j;
}

// Every level's factors and spikes, top down, from the operator's current values (creation and
// vtk_prec_refresh).  VTK_ERR_SINGULAR: a zero or non-finite pivot at some level (the first such
// level's smallest row is named).
int linec_factor(vtk_prec *M) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    const LineC &C = M->linec;
    if (C.n <= 0) return VTK_OK;
    DBuf bad, co;
    std::vector<unsigned long long> hb((size_t)C.nlev + 1, ~0ull);
    TRY(dalloc(c, bad, hb.size() * sizeof(unsigned long long)));
    TRY(dalloc(c, co, 3 * (size_t)std::max<int64_t>(C.lev[1].n, 1) * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(bad.p, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < C.nlev; ++k) {
        Prof pf(c, "linec_setup", -1, (k == 0 ? matrix_bytes(A) : 24.0 * (double)C.lev[k].n) + 72.0 * (double)C.lev[k].n);
        HIPCHK(c, launch_linec_setup(A->d_indptr, A->d_indices, A->d_data, A->fp32, C, k, co.as<double>(),
                                     bad.as<unsigned long long>(), c->stream));
    }
    if (c->prof_on) prof_flush(c);
    HIPCHK(c, hipMemcpyAsync(hb.data(), bad.p, hb.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k <= C.nlev; ++k) {
        if (hb[k] == ~0ull) continue;
        // the last level's pivot belongs to its separator, the line's last unknown
        const int lev = std::min(k, C.nlev - 1);
        const int64_t idx = k < C.nlev ? (int64_t)hb[k]
                                       : ((int64_t)hb[k] / C.stride * C.lev[lev].period + C.lev[lev].period - 1) * C.stride + (int64_t)hb[k] % C.stride;
        return fail(c, VTK_ERR_SINGULAR, "vtk_linecyclic_create: zero or non-finite pivot at row " + std::to_string(linec_row(C, lev, idx)) +
                                             " (level " + std::to_string(lev) + ")");
    }
    return VTK_OK;
}

// ---- the registry of live preconditioners (a Neumann wrapper borrows its base) ------------------
namespace {
std::mutex g_live_mu;
std::unordered_map<const vtk_prec *, uint64_t> g_live;
uint64_t g_next_id = 1;
}  // namespace

void prec_register(vtk_prec *M) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    M->id = g_next_id++;
    g_live[M] = M->id;
}

void prec_unregister(const vtk_prec *M) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.erase(M);
}

// the address still holds the preconditioner that had this serial (not a later one at the same
// place); id 0: any live preconditioner at this address (a handle the caller just passed in)
bool prec_alive(const vtk_prec *M, uint64_t id) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    const auto it = g_live.find(M);
    return it != g_live.end() && (id == 0 || it->second == id);
}

// a preconditioner whose last vtk_prec_refresh met a singular block has no factors to apply or
// export (the old ones are overwritten): VTK_ERR_STATE until a refresh succeeds.  A Neumann wrapper
// is as usable as its base, which must still exist
int prec_usable(const vtk_prec *M, const char *who) {
    if (!M) return VTK_OK;
    if (M->kind == VTK_PREC_NEUMANN) {
        if (!prec_alive(M->base, M->base_id))
            return fail(M->A->ctx, VTK_ERR_STATE, std::string(who) + ": the Neumann wrapper's base preconditioner has been "
                                                                       "destroyed (the wrapper borrows it)");
        return prec_usable(M->base, who);
    }
    if (M->valid) return VTK_OK;
    return fail(M->A->ctx, VTK_ERR_STATE, std::string(who) + ": the preconditioner's last refresh failed (singular); "
                                                               "refresh it from non-singular values first");
}

// ---- z = M^-1 r for every kind; the Neumann wrapper's corrections ---------------
namespace {

// a launch of an apply: voted across ranks inside a solve, else returned at once
int neu_launch(vtk_ctx *c, Vote *vote, hipError_t e, const char *what) {
    if (vote) return vote->launch(e, what);
    if (e == hipSuccess) return VTK_OK;
    return fail(c, e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define NSOFT(x) TRY(neu_launch(c, vote, (x), #x))

// N_k^-1 r: z_1 = M^-1 r, then k - 1 corrections z <- z + M^-1 (r - A z); the last one writes z and
// the partials (or the step's dots) the caller asked for.  z_i alternate between two of the wrapper's
// vectors, t = r - A z_i lives in the third
int neumann_apply(vtk_prec *N, int64_t n, const double *r, double *z, const double *v0, double *part0, double *part1,
                  int grid, const int *stop, int col, Vote *vote, const StepDots *dots, int *cnt) {
    vtk_prec *B = N->base;
    vtk_csr *A = N->A;
    vtk_ctx *c = A->ctx;
    const int k = N->degree;
    const BjOp bop = bj_op(B);
    const double n8 = 8.0 * (double)n, b_base = bj_row_bytes(B) * (double)n, b_mat = solver_matrix_bytes(A);
    if (k == 1) {   // the base, bit for bit
        Prof pf(c, prec_cls(B), col, b_base + 2 * n8);
        NSOFT(launch_bj_apply(bop, n, r, z, v0, part0, part1, grid, stop, col, c->stream));
        return VTK_OK;
    }
    if (r == z) return fail(c, VTK_ERR_ARG, "Neumann wrapper: the apply's input and output must not alias");
    const int64_t ld = round_up(std::max<int64_t>(n, 1), 64);
    double *cur = N->d_neu, *oth = cur + ld, *t = oth + ld;
    { Prof pf(c, prec_cls(B), col, b_base + 2 * n8);
      NSOFT(launch_bj_apply(bop, n, r, cur, nullptr, nullptr, nullptr, grid, stop, col, c->stream)); }
    const bool fuse = neu_fused(N);
    const double b_fused = (bop.tri ? 24.0 : 8.0 * B->bs) * (double)n;   // the stored l | m | g, or the inverse rows
    for (int i = 1; i < k; ++i) {
        const bool last = i == k - 1;
        double *out = last ? z : oth;
        const double *lv0 = last ? v0 : nullptr;
        double *lp0 = last ? part0 : nullptr, *lp1 = last ? part1 : nullptr;
        const StepDots *ld_ = last ? dots : nullptr;
        TRY(halo_exchange(A, cur));
        const SpmvIn in = lsv_in(spmv_in(A, fuse ? &B->tiles : &A->tiles, cur), A);
        // one launch: w = z + M^-1 (r - A z).  Its partials come per SpMV workgroup: zero-padded up
        // to the caller's count; a launch with more workgroups than that (operators of fewer than
        // 512 GMAX rows) leaves them to the dot kernel
        if (fuse) {
            const int g = spmv_grid(in);
            const bool own = lp0 && g <= grid;
            { Prof pf(c, "neu_corr", col, b_mat + b_fused + 3 * n8);
              NSOFT(launch_spmv(in, EPI_NEU_CORR, out, r, bop, own ? lv0 : nullptr, own ? lp0 : nullptr, own ? lp1 : nullptr,
                                stop, col, c->stream)); }
            if (own && g < grid) {
                HIPCHK(c, hipMemsetAsync(lp0 + g, 0, (size_t)(grid - g) * sizeof(double), c->stream));
                if (lp1 && lv0) HIPCHK(c, hipMemsetAsync(lp1 + g, 0, (size_t)(grid - g) * sizeof(double), c->stream));
            }
            if (lp0 && !own) {
                Prof pf(c, "dot", col, (lp1 && lv0 ? 3 : 1) * n8);
                NSOFT(launch_dot(out, nullptr, n, lp0, grid, c->stream));
                if (lp1 && lv0) NSOFT(launch_dot(lv0, out, n, lp1, grid, c->stream));
            }
        } else {
            { Prof pf(c, "neu_resid", col, b_mat + 3 * n8);
              const SpmvIn rin = lsv_in(spmv_in(A, &A->tiles, cur), A);
              NSOFT(launch_spmv(rin, EPI_NEU_RESID, t, r, BjOp{}, nullptr, nullptr, nullptr, stop, col, c->stream)); }
            // the step's dots behind the last write, where the kind's kernel has that form
            const bool dc = ld_ && c->tune.neu_dc && grid <= GMAX && ld_->j <= DC_MAXJ;
            const double b_dc = dc ? n8 * (ld_->j + 1) : 0.0;   // p and V_j
            if (B->kind == VTK_PREC_LINE) {
                const LineOp &L = B->line;
                Prof pf(c, "neu_corr", col, b_base + 3 * n8 + b_dc);
                if (dc && L.seg >= 1 && L.seg <= 32) {
                    NSOFT(launch_line_dc(L, t, out, ld_->V, ld_->ld, ld_->j, ld_->V + (size_t)ld_->j * ld_->ld, ld_->part, grid,
                                         stop, col, c->stream, cur));
                    *cnt = grid;
                } else {
                    NSOFT(launch_line_apply(L, t, out, lv0, lp0, lp1, grid, stop, col, c->stream, cur));
                }
            } else if (B->kind == VTK_PREC_LINE2) {
                { Prof pf(c, "line_apply", col, line_row_bytes(B->line) * (double)n + 2 * n8);   // t = M1^-1 t in place
                  NSOFT(launch_line_apply(B->line, t, t, nullptr, nullptr, nullptr, grid, stop, col, c->stream)); }
                const LineOp &L2 = B->line2;
                Prof pf(c, "neu_corr", col, (line_row_bytes(L2) + 8.0) * (double)n + 3 * n8 + b_dc);
                if (dc && L2.seg >= 1 && L2.seg <= 32) {
                    NSOFT(launch_line2_dc(L2, B->d_diag, t, out, ld_->V, ld_->ld, ld_->j, ld_->V + (size_t)ld_->j * ld_->ld,
                                          ld_->part, grid, stop, col, c->stream, cur));
                    *cnt = grid;
                } else {
                    NSOFT(launch_line2_apply(L2, B->d_diag, t, out, lv0, lp0, lp1, grid, stop, col, c->stream, cur));
                }
            } else if (B->kind == VTK_PREC_LINEC) {
                const LineC &C = B->linec;
                { Prof pf(c, "linec_sweep", col, linec_sweep_bytes(C));
                  NSOFT(launch_linec_phase(C, 0, t, out, nullptr, nullptr, nullptr, grid, stop, col, c->stream)); }
                { Prof pf(c, "linec_reduced", col, linec_reduced_bytes(C));
                  NSOFT(launch_linec_phase(C, 1, t, out, nullptr, nullptr, nullptr, grid, stop, col, c->stream)); }
                Prof pf(c, "neu_corr", col, linec_correct_bytes(C) + n8);
                NSOFT(launch_linec_phase(C, 2, t, out, lv0, lp0, lp1, grid, stop, col, c->stream, cur));
            } else {   // block Jacobi off the fused tiles: u = M^-1 t into `out`, then w = z + u in place
                { Prof pf(c, "bj_apply", col, b_base + 2 * n8);
                  NSOFT(launch_bj_apply(bop, n, t, out, nullptr, nullptr, nullptr, grid, stop, col, c->stream)); }
                Prof pf(c, "neu_corr", col, 3 * n8 + b_dc);
                if (dc) {
                    NSOFT(launch_neu_add_dc(cur, out, out, n, ld_->V, ld_->ld, ld_->j, ld_->part, grid, stop, col, c->stream));
                    *cnt = grid;
                } else {
                    NSOFT(launch_neu_add(cur, out, out, n, lv0, lp0, lp1, grid, stop, col, c->stream));
                }
            }
        }
        if (!last) std::swap(cur, oth);
    }
    return VTK_OK;
}
#undef NSOFT

}  // namespace

int prec_apply(vtk_ctx *c, vtk_prec *M, int64_t n, const double *r, double *z, const double *v0, double *part0,
               double *part1, int grid, const int *stop_col, int col, Vote *vote, const StepDots *dots, int *cnt) {
    int none = 0;
    if (!cnt) cnt = &none;
    *cnt = 0;
    if (M && M->kind == VTK_PREC_NEUMANN)
        return neumann_apply(M, n, r, z, v0, part0, part1, grid, stop_col, col, vote, dots, cnt);
    return neu_launch(c, vote, launch_bj_apply(bj_op(M), n, r, z, v0, part0, part1, grid, stop_col, col, c->stream),
                      "launch_bj_apply");
}

}  // namespace vtk
