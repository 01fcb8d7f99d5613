// vtk_precond.cpp -- preconditioner factors from the operator's current values: block Jacobi, line
// Jacobi, the two-direction line product, the periodic whole lines (vtk_*_create and vtk_prec_refresh call these).
#include <climits>

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

// a preconditioner whose last vtk_prec_refresh met a singular block has no factors to apply or
// export (the old ones are overwritten): VTK_ERR_STATE until a refresh succeeds
int prec_usable(const vtk_prec *M, const char *who) {
    if (!M || M->valid) return VTK_OK;
    return fail(M->A->ctx, VTK_ERR_STATE, std::string(who) + ": the preconditioner's last refresh failed (singular); "
                                                               "refresh it from non-singular values first");
}

}  // namespace vtk
