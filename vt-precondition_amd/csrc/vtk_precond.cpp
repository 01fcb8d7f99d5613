// vtk_precond.cpp -- preconditioner factors from the operator's current values (block Jacobi, line
// Jacobi, the two-direction line product, the periodic whole lines and their span over the ranks:
// vtk_*_create and vtk_prec_refresh call these), the plans of the cyclic lines, and the registry of
// live preconditioners.  Applying the factors: vtk_apply.cpp.
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
    for (void *p : {(void *)C.sp.vw, (void *)C.sp.ecol, (void *)C.sp.tsend, (void *)C.sp.tips, (void *)C.sp.edge,
                    (void *)C.sp.edges, (void *)C.sp.xe})
        (void)hipFree(p);
    C.sp = LineCSpan{};
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
static int linec_factor_local(vtk_prec *M) {
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
        return fail(c, VTK_ERR_SINGULAR, std::string(C.sp.on ? "vtk_linecyclic_create_span" : "vtk_linecyclic_create") +
                                             ": zero or non-finite pivot at row " + std::to_string(linec_row(C, lev, idx)) +
                                             " (level " + std::to_string(lev) + ")");
    }
    return VTK_OK;
}

// ---- lines that span the ranks (vtk_linecyclic_create_span) -----------------------
// The plan: collective.  Every rank contributes (row count, first row, whether its own arguments
// hold); the decision is made from the gathered table, the same on every rank, after the collective.
// Then the levels of the rank's open chunk (linec_plan with period P_p, one block) and the rank
// level's storage.
static int linec_span_storage(vtk_prec *M, int64_t stride, int64_t period, int64_t seg);
int linec_span_plan(vtk_prec *M, int64_t stride, int64_t period, int64_t seg) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    const int W = c->dist ? c->world : 1;
    if (W > LINEC_SPAN_MAXW)   // (the same on every rank: no collective is entered)
        return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create_span: at most " + std::to_string(LINEC_SPAN_MAXW) + " ranks");
    const bool args = stride >= 1 && period >= 3 && seg >= 2 && stride <= INT64_MAX / period && A->n_global == stride * period;
    std::vector<int64_t> all{A->n_local, A->row_begin, args ? 1 : 0};
    if (c->dist) {
        int64_t *mine = reinterpret_cast<int64_t *>(c->d_scal + 128);   // the scalar scratch: no allocation that could fail on one rank only
        HIPCHK(c, hipMemcpyAsync(mine, all.data(), 3 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        TRY(comm_allgather_i64(c, mine, mine + 3, 3));
        all.resize(3 * (size_t)W);
        HIPCHK(c, hipMemcpyAsync(all.data(), mine + 3, all.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int q = 0; q < W; ++q)
        if (!all[3 * q + 2])
            return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create_span: stride must be >= 1, period >= 3, seg >= 2 and "
                                        "n_global == stride * period (one block of lines)");
    for (int q = 0; q < W; ++q)
        if (all[3 * q] % stride != 0 || all[3 * q + 1] % stride != 0 || all[3 * q] / stride < 3)
            return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create_span: rank " + std::to_string(q) + "'s first row and row count "
                                        "must be multiples of stride, with at least 3 line indices per rank");
    // the storage: a failure on one rank only (an allocation) must not leave the peers in the tips
    // gather that follows, so every rank's verdict is gathered first (the scalar scratch again)
    const int arc = linec_span_storage(M, stride, period, seg);
    std::vector<int64_t> vr{arc};
    if (c->dist) {
        int64_t *mine = reinterpret_cast<int64_t *>(c->d_scal + 128);
        HIPCHK(c, hipMemcpyAsync(mine, vr.data(), sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        TRY(comm_allgather_i64(c, mine, mine + 1, 1));
        vr.resize((size_t)W);
        HIPCHK(c, hipMemcpyAsync(vr.data(), mine + 1, vr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (arc != VTK_OK) return arc;   // (its message stands)
    for (int q = 0; q < W; ++q)
        if (vr[q] != VTK_OK)
            return fail(c, VTK_ERR_PEER, "vtk_linecyclic_create_span: rank " + std::to_string(q) + " could not set up its storage (" +
                                             vtk_status_string((int)vr[q]) + "); every rank left the creation there");
    return VTK_OK;
}

// the levels of the rank's chunk and the rank level's storage (local; linec_span_plan gathers the verdict)
static int linec_span_storage(vtk_prec *M, int64_t stride, int64_t period, int64_t seg) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    const int W = c->dist ? c->world : 1, me = c->dist ? c->rank : 0;
    const int64_t Pp = A->n_local / stride;
    TRY(linec_plan(M, stride, Pp, seg));
    LineC &C = M->linec;
    LineCSpan &sp = C.sp;
    sp.on = true;
    sp.world = W;
    sp.rank = me;
    sp.gperiod = period;
    sp.i0 = A->row_begin / stride;
    const size_t S = (size_t)stride;
    HIPCHK(c, hipMalloc(&sp.vw, 2 * (size_t)C.n * sizeof(double)));
    HIPCHK(c, hipMalloc(&sp.ecol, 2 * S * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&sp.tsend, (4 * S + 1) * sizeof(double)));
    HIPCHK(c, hipMalloc(&sp.tips, (size_t)W * (4 * S + 1) * sizeof(double)));
    HIPCHK(c, hipMalloc(&sp.edge, 2 * S * sizeof(double)));
    HIPCHK(c, hipMalloc(&sp.edges, (size_t)W * 2 * S * sizeof(double)));
    HIPCHK(c, hipMalloc(&sp.xe, 2 * S * sizeof(double)));
    // where the CSR keeps the couplings to the neighbour ranks' edge rows: the local column of the
    // global row (i0 - 1) stride + j (a_first) and (i0 + P_p) stride + j (c_last), modulo the period;
    // owned columns come first, the halo's follow in ascending global order
    std::vector<int32_t> ec(2 * S, -1);
    const int64_t gl = ((sp.i0 - 1 + period) % period) * stride, gr = ((sp.i0 + Pp) % period) * stride;
    for (int w = 0; w < 2; ++w)
        for (int64_t j = 0; j < stride; ++j) {
            const int64_t g = (w ? gr : gl) + j;
            if (g >= A->row_begin && g < A->row_end) {
                ec[w * S + j] = (int32_t)(g - A->row_begin);
            } else {
                const auto it = std::lower_bound(A->halo_cols.begin(), A->halo_cols.end(), g);
                if (it != A->halo_cols.end() && *it == g) ec[w * S + j] = (int32_t)(A->n_local + (it - A->halo_cols.begin()));
            }
        }
    HIPCHK(c, hipMemcpy(sp.ecol, ec.data(), ec.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return VTK_OK;
}

// The factors of lines that span the ranks: collective.  The chunk's levels, V_p and W_p by two
// applications of the local solver, the tips gathered with a flag slot (a rank whose chunk has a
// zero pivot still joins the gather; every rank then returns VTK_ERR_SINGULAR; after any other
// failure of one rank the others return VTK_ERR_PEER), the interface
// system's pivots checked by its own kernel (identical data, the same verdict on every rank).
static int linec_span_factor(vtk_prec *M) {
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    LineC &C = M->linec;
    const LineCSpan &sp = C.sp;
    const int64_t S = C.stride, tq = 4 * S + 1;
    // this rank's part; whatever it returns, the rank joins the gather below with its verdict in
    // the flag slot (0, 1: a zero pivot, 2: any other failure), so that no peer waits in it alone
    int rc = linec_factor_local(M);
    if (rc == VTK_OK)
        rc = [&]() -> int {
            DBuf rhs;
            TRY(dalloc(c, rhs, (size_t)C.n * sizeof(double)));
            for (int w = 0; w < 2; ++w) {
                Prof pf(c, "linec_setup", -1, 16.0 * (double)C.n + prec_row_bytes(M) * (double)C.n);
                HIPCHK(c, launch_linec_span_rhs(A->d_indptr, A->d_indices, A->d_data, A->fp32, C, w, rhs.as<double>(), c->stream));
                Apply ap{rhs.as<double>(), sp.vw + (size_t)w * C.n};
                ap.grid = vector_grid(C.n);
                ap.chunk = true;
                TRY(kind_apply(c, M, C.n, ap));
            }
            HIPCHK(c, launch_linec_span_tips(C, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));   // rhs is freed here
            return VTK_OK;
        }();
    const std::string own = rc == VTK_OK ? std::string() : c->err;
    const double flag = rc == VTK_OK ? 0.0 : rc == VTK_ERR_SINGULAR ? 1.0 : 2.0;
    HIPCHK(c, hipMemcpyAsync(sp.tsend + 4 * S, &flag, sizeof(double), hipMemcpyHostToDevice, c->stream));
    TRY(comm_allgather(c, sp.tsend, sp.tips, tq));
    std::vector<double> fl((size_t)sp.world, 0.0);
    HIPCHK(c, hipMemcpy2DAsync(fl.data(), sizeof(double), sp.tips + 4 * S, (size_t)tq * sizeof(double), sizeof(double),
                               (size_t)sp.world, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (rc != VTK_OK) return fail(c, rc, own);
    for (int q = 0; q < sp.world; ++q) {
        if (fl[q] == 1.0)
            return fail(c, VTK_ERR_SINGULAR, "vtk_linecyclic_create_span: rank " + std::to_string(q) +
                                                 " met a zero or non-finite pivot in its chunk of the lines");
        if (fl[q] != 0.0)
            return fail(c, VTK_ERR_PEER, "vtk_linecyclic_create_span: rank " + std::to_string(q) +
                                             " failed while factoring its chunk; every rank left there");
    }
    // the interface system's pivots (they do not depend on the edge values: zeros)
    DBuf bad;
    TRY(dalloc(c, bad, sizeof(unsigned long long)));
    const unsigned long long none = ~0ull;
    unsigned long long hb = none;
    HIPCHK(c, hipMemcpyAsync(bad.p, &none, sizeof(none), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(sp.edges, 0, (size_t)sp.world * 2 * S * sizeof(double), c->stream));
    HIPCHK(c, launch_linec_span_iface(C, bad.as<unsigned long long>(), nullptr, 0, c->stream));
    TRY(read_back(c, hb, bad.p));
    if (hb != none)
        return fail(c, VTK_ERR_SINGULAR, "vtk_linecyclic_create_span: the interface system of the ranks is singular (zero or "
                                         "non-finite pivot) on line " + std::to_string(hb));
    return VTK_OK;
}

int linec_factor(vtk_prec *M) { return M->linec.sp.on ? linec_span_factor(M) : linec_factor_local(M); }

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

}  // namespace vtk
