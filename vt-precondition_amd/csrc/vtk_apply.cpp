// vtk_apply.cpp -- z = M^-1 r: the launches of every preconditioner kind, each kind's sequence once
// (kind_apply), the Neumann wrapper's corrections around them, and next to the launches
// their profile classes and byte models.  The factors they read: vtk_precond.cpp.
#include "vtk_driver.hpp"

using namespace vtk;

namespace vtk {

// ---- profile classes and byte models -----------------------------------------------------------
const char *prec_cls(const vtk_prec *M) {
    if (M && M->kind == VTK_PREC_NEUMANN) return nullptr;
    if (M && M->kind == VTK_PREC_LINEC) return "linec_apply";   // the three phases of the cyclic lines
    if (M && M->kind == VTK_PREC_LINE2) return "line2_apply";   // both sweeps of the product
    return M && M->kind == VTK_PREC_LINE ? "line_apply" : "bj_apply";
}

namespace {

// bytes per row of one direction's factors as a sweep reads them: m (compact) or l, m, g
double line_row_bytes(const LineOp &L) { return L.compact ? 8.0 : 24.0; }

// periodic whole lines, algorithmic bytes of the three phases: the level-0 sweep
// reads r, l, m, g and writes y; the reduced part gathers per separator (r_s, a_s, c_s, two y read,
// one value written) and runs every reduced level in place (sweep 40 B, correction 32 B per unknown,
// its own gather; the last level's one lane per line reads its five factor rows); the level-0
// correction reads y, V, W and the separator values and writes z
double linec_sweep_bytes(const LineC &C) { return 40.0 * (double)C.n; }
double linec_reduced_bytes(const LineC &C) {
    double b = C.nlev > 1 ? 48.0 * (double)C.lev[1].n : 0.0;
    for (int k = 1; k < C.nlev; ++k) b += (k + 1 < C.nlev ? 72.0 + 48.0 * (double)C.lev[k + 1].n / (double)std::max<int64_t>(C.lev[k].n, 1) : 88.0) * (double)C.lev[k].n;
    return b;
}
double linec_correct_bytes(const LineC &C) { return 32.0 * (double)C.n + (C.nlev > 1 ? 8.0 * (double)C.lev[1].n : 0.0); }
// lines that span the ranks: the fused correction also reads V_p and W_p; the rank
// level between phases 1 and 3 writes two edge values per line (five reads), gathers 16 B per line
// and rank, and solves the interface system from every rank's four tips and two edge values
double linec_correct_span_bytes(const LineC &C) { return linec_correct_bytes(C) + 16.0 * (double)C.n; }
double linec_span_bytes(const LineC &C) { return (56.0 + (16.0 + 48.0) * (double)C.sp.world + 16.0) * (double)C.stride; }

}  // namespace

double prec_row_bytes(const vtk_prec *M, bool tri_stored) {
    if (!M) return 0.0;
    switch (M->kind) {
        // the wrapper: `degree` applications of the base; per correction the residual (the matrix, z and
        // r read, t written), the base's own t read and u written, and the addition (z and u read, w
        // written; fused into the base's last write where the kind allows -- the model keeps the
        // unfused figure)
        case VTK_PREC_NEUMANN: {
            const double nn = (double)std::max<int64_t>(M->A->n_local, 1);
            return M->degree * prec_row_bytes(M->base) + (M->degree - 1) * (solver_matrix_bytes(M->A) / nn + 24.0 + 16.0 + 24.0);
        }
        case VTK_PREC_LINE: return line_row_bytes(M->line);
        // the product: both directions' factors, D, and t = M1^-1 r written and read back
        case VTK_PREC_LINE2: return line_row_bytes(M->line) + line_row_bytes(M->line2) + 8.0 + 16.0;
        case VTK_PREC_LINEC: {   // the phases' bytes (summed in launch order: linec_reduced_bytes divides)
            const LineC &C = M->linec;
            const double b = linec_sweep_bytes(C) + linec_reduced_bytes(C);
            return (C.sp.on ? b + linec_span_bytes(C) + linec_correct_span_bytes(C) : b + linec_correct_bytes(C)) /
                       (double)std::max<int64_t>(C.n, 1) - 16.0;
        }
        default: break;
    }
    if (bj_op(M).tri) return M->A->use_sell && !tri_stored ? 8.0 : 24.0;   // (the SELL kernels read only m)
    return 8.0 * M->bs;
}

// ---- one apply of a non-wrapper kind -----------------------------------------------------------
// prof: the kind's own classes, launch by launch.  Where the step's dots are asked for and the kind's
// last kernel has a dots form (line sweeps in registers: segments <= 32; the addition behind block
// Jacobi), that form runs and *cnt = grid; the byte models count p and V_j whenever they were asked for
int kind_apply(vtk_ctx *c, vtk_prec *M, int64_t n, const Apply &a, int *cnt) {
    int none = 0;
    if (!cnt) cnt = &none;
    *cnt = 0;
    hipStream_t s = c->stream;
    const StepDots *d = a.dots;
    const double *pj = d ? d->V + (size_t)d->j * d->ld : nullptr;
    const double n8 = 8.0 * (double)n, b_acc = a.acc ? n8 : 0.0, b_dots = d ? n8 * (d->j + 1) : 0.0;
    const auto mid = [&](const char *own) { return a.prof ? own : nullptr; };
    const auto last = [&](const char *own) { return a.prof && a.last_cls ? a.last_cls : mid(own); };
#define ASOFT(x) SOFT_LAUNCH(c, a.vote, x)
    switch (M ? M->kind : VTK_PREC_BJACOBI) {
        case VTK_PREC_BJACOBI: {
            const BjOp bj = bj_op(M);
            const double b_bj = prec_row_bytes(M) * (double)n + 2 * n8;
            if (!a.acc) {
                Prof pf(c, last("bj_apply"), a.col, b_bj);
                ASOFT(launch_bj_apply(bj, n, a.r, a.z, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s));
                return VTK_OK;
            }
            // no kernel of its own adds: u = M^-1 r into z, then z = acc + u in place
            { Prof pf(c, mid("bj_apply"), a.col, b_bj);
              ASOFT(launch_bj_apply(bj, n, a.r, a.z, nullptr, nullptr, nullptr, a.grid, a.stop, a.col, s)); }
            Prof pf(c, last("neu_add"), a.col, 3 * n8 + b_dots);
            if (d) {
                ASOFT(launch_neu_add_dc(a.acc, a.z, a.z, n, d->V, d->ld, d->j, d->part, a.grid, a.stop, a.col, s));
                *cnt = a.grid;
            } else {
                ASOFT(launch_neu_add(a.acc, a.z, a.z, n, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s));
            }
            return VTK_OK;
        }
        case VTK_PREC_LINE: {
            const LineOp &L = M->line;
            const bool dc = d && L.seg >= 1 && L.seg <= 32;
            Prof pf(c, last(dc ? "line_dc" : "line_apply"), a.col, line_row_bytes(L) * (double)n + 2 * n8 + b_acc + b_dots);
            if (dc) {
                ASOFT(launch_line_dc(L, a.r, a.z, d->V, d->ld, d->j, pj, d->part, a.grid, a.stop, a.col, s, a.acc));
                *cnt = a.grid;
            } else {
                ASOFT(launch_line_apply(L, a.r, a.z, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s, a.acc));
            }
            return VTK_OK;
        }
        case VTK_PREC_LINE2: {   //  t = M1^-1 r into z, then z = M2^-1 (D t) in place
            const LineOp &L2 = M->line2;
            { Prof pf(c, mid("line_apply"), a.col, line_row_bytes(M->line) * (double)n + 2 * n8);
              ASOFT(launch_line_apply(M->line, a.r, a.z, nullptr, nullptr, nullptr, a.grid, a.stop, a.col, s)); }
            const bool dc = d && L2.seg >= 1 && L2.seg <= 32;
            Prof pf(c, last(dc ? "line2_dc" : "line2_sweep"), a.col, (line_row_bytes(L2) + 8.0) * (double)n + 2 * n8 + b_acc + b_dots);   // t, D, m, z
            if (dc) {
                ASOFT(launch_line2_dc(L2, M->d_diag, a.z, a.z, d->V, d->ld, d->j, pj, d->part, a.grid, a.stop, a.col, s, a.acc));
                *cnt = a.grid;
            } else {
                ASOFT(launch_line2_apply(L2, M->d_diag, a.z, a.z, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s, a.acc));
            }
            return VTK_OK;
        }
        case VTK_PREC_LINEC: {   //  the level-0 sweep, the reduced levels, the level-0 correction
            const LineC &C = M->linec;
            const bool span = C.sp.on && !a.chunk;
            if (span && a.acc) return fail(c, VTK_ERR_ARG, "cyclic lines that span the ranks: no apply with an addend");
            { Prof pf(c, mid("linec_sweep"), a.col, linec_sweep_bytes(C));
              ASOFT(launch_linec_phase(C, 0, a.r, a.z, nullptr, nullptr, nullptr, a.grid, a.stop, a.col, s)); }
            { Prof pf(c, mid("linec_reduced"), a.col, linec_reduced_bytes(C));
              ASOFT(launch_linec_phase(C, 1, a.r, a.z, nullptr, nullptr, nullptr, a.grid, a.stop, a.col, s)); }
            if (!span) {
                Prof pf(c, last("linec_correct"), a.col, linec_correct_bytes(C) + b_acc);
                ASOFT(launch_linec_phase(C, 2, a.r, a.z, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s, a.acc));
                return VTK_OK;
            }
            // the rank level: the two edge values per line, one gather, the interface
            // system, the fused correction.  Every rank issues the gather at every call (inside a solve
            // also after the stop column, where the kernels return at entry); a failed collective
            // returns at once
            { Prof pf(c, mid("linec_span"), a.col, linec_span_bytes(C));
              ASOFT(launch_linec_span_edge(C, a.z, a.stop, a.col, s));
              TRY(comm_allgather(c, C.sp.edge, C.sp.edges, 2 * C.stride));
              ASOFT(launch_linec_span_iface(C, nullptr, a.stop, a.col, s)); }
            Prof pf(c, last("linec_correct_span"), a.col, linec_correct_span_bytes(C));
            ASOFT(launch_linec_span_correct(C, a.z, a.v0, a.part0, a.part1, a.grid, a.stop, a.col, s));
            return VTK_OK;
        }
        default: return fail(c, VTK_ERR_ARG, "kind_apply: no launch sequence for preconditioner kind " + std::to_string(M->kind));
    }
#undef ASOFT
}

// ---- the Neumann wrapper --------------------------------------------------------
// N_k^-1 r: z_1 = M^-1 r, then k - 1 corrections z <- z + M^-1 (r - A z); the last one writes z and
// the partials (or the step's dots) the caller asked for.  z_i alternate between two of the wrapper's
// vectors, t = r - A z_i lives in the third
static int neumann_apply(vtk_prec *N, int64_t n, const Apply &a, int *cnt) {
    vtk_prec *B = N->base;
    vtk_csr *A = N->A;
    vtk_ctx *c = A->ctx;
    const int k = N->degree;
    const double n8 = 8.0 * (double)n, b_base = prec_row_bytes(B) * (double)n, b_mat = solver_matrix_bytes(A);
    Apply first = a;   // z_1: the base's whole apply under its standalone class
    first.dots = nullptr;
    if (k == 1) {   // the base, bit for bit
        Prof pf(c, prec_cls(B), a.col, b_base + 2 * n8);
        return kind_apply(c, B, n, first);
    }
    if (a.r == a.z) return fail(c, VTK_ERR_ARG, "Neumann wrapper: the apply's input and output must not alias");
    const int64_t ld = round_up(std::max<int64_t>(n, 1), 64);
    double *cur = N->d_neu, *oth = cur + ld, *t = oth + ld;
    first.z = cur;
    first.v0 = nullptr;
    first.part0 = first.part1 = nullptr;
    { Prof pf(c, prec_cls(B), a.col, b_base + 2 * n8);
      TRY(kind_apply(c, B, n, first)); }
    const bool fuse = neu_fused(N);
    const BjOp bop = bj_op(B);
    const double b_fused = (bop.tri ? 24.0 : 8.0 * B->bs) * (double)n;   // the stored l | m | g, or the inverse rows
    for (int i = 1; i < k; ++i) {
        const bool last = i == k - 1;
        Apply co = last ? a : first;   // w = cur + M^-1 t, its launches profiled one by one, the last as neu_corr
        co.z = last ? a.z : oth;
        co.acc = cur;
        co.prof = true;
        co.last_cls = "neu_corr";
        TRY(halo_exchange(A, cur));
        // one launch: w = z + M^-1 (r - A z).  Its partials come per SpMV workgroup: zero-padded up
        // to the caller's count; a launch with more workgroups than that (operators of fewer than
        // 512 GMAX rows) leaves them to the dot kernel
        if (fuse) {
            const SpmvIn in = lsv_in(spmv_in(A, &B->tiles, cur), A);
            const int g = spmv_grid(in);
            const bool own = co.part0 && g <= a.grid;
            { Prof pf(c, "neu_corr", a.col, b_mat + b_fused + 3 * n8);
              SOFT_LAUNCH(c, a.vote, launch_spmv(in, EPI_NEU_CORR, co.z, a.r, bop, own ? co.v0 : nullptr, own ? co.part0 : nullptr,
                                                 own ? co.part1 : nullptr, a.stop, a.col, c->stream)); }
            if (own && g < a.grid) {
                HIPCHK(c, hipMemsetAsync(co.part0 + g, 0, (size_t)(a.grid - g) * sizeof(double), c->stream));
                if (co.part1 && co.v0) HIPCHK(c, hipMemsetAsync(co.part1 + g, 0, (size_t)(a.grid - g) * sizeof(double), c->stream));
            }
            if (co.part0 && !own) {
                Prof pf(c, "dot", a.col, (co.part1 && co.v0 ? 3 : 1) * n8);
                SOFT_LAUNCH(c, a.vote, launch_dot(co.z, nullptr, n, co.part0, a.grid, c->stream));
                if (co.part1 && co.v0) SOFT_LAUNCH(c, a.vote, launch_dot(co.v0, co.z, n, co.part1, a.grid, c->stream));
            }
        } else {
            { Prof pf(c, "neu_resid", a.col, b_mat + 3 * n8);
              const SpmvIn rin = lsv_in(spmv_in(A, &A->tiles, cur), A);
              SOFT_LAUNCH(c, a.vote, launch_spmv(rin, EPI_NEU_RESID, t, a.r, BjOp{}, nullptr, nullptr, nullptr, a.stop, a.col, c->stream)); }
            co.r = t;
            // the step's dots behind the last write, where the kind's kernel has that form
            if (co.dots && !(c->tune.neu_dc && a.grid <= GMAX && co.dots->j <= DC_MAXJ)) co.dots = nullptr;
            TRY(kind_apply(c, B, n, co, cnt));
        }
        if (!last) std::swap(cur, oth);
    }
    return VTK_OK;
}

int prec_apply(vtk_ctx *c, vtk_prec *M, int64_t n, const double *r, double *z, const double *v0, double *part0,
               double *part1, int grid, const int *stop_col, int col, Vote *vote, const StepDots *dots, int *cnt) {
    if (cnt) *cnt = 0;
    Apply a{r, z};
    a.v0 = v0, a.part0 = part0, a.part1 = part1;
    a.grid = grid, a.stop = stop_col, a.col = col, a.vote = vote;
    if (!M || M->kind != VTK_PREC_NEUMANN) return kind_apply(c, M, n, a);
    a.dots = dots;
    return neumann_apply(M, n, a, cnt);
}

}  // namespace vtk
