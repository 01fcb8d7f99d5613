// vtk_bicg.cpp -- the BiCGStab driver.
//
// scipy.sparse.linalg.bicgstab (iterative.py) with every vector operation, every reduction and
// every test of the loop on the device (vtk_bicgstab.hip).  The host enqueues whole
// iterations, LOOKAHEAD of them ahead of the device, and watches the mapped stop flag; kernels
// tagged after the stop return at entry.  Across ranks (vtk_ctx::dist) the sums are all-reduced as
// small records that carry a failure vote (k_bcg_reduce; DESIGN.md §3j, "Across ranks").
#include <climits>

#include "vtk_driver.hpp"

using namespace vtk;

namespace {

static_assert(sizeof(BicgState) <= sizeof(GmresState), "the pinned state mirror holds either solver's record");

const Red none{nullptr, 0};

// one solve: its operands (set by run_bicgstab), what follows from them, and the pieces of its schedule
struct Bicg {
    vtk_csr *A;
    vtk_prec *M;
    vtk_ctx *c;
    const double *b;
    double *x;
    int info_max;
    double atol = 0.0;
    int64_t n = A->n_local, ld = round_up(std::max<int64_t>(n, 1), 64);
    int G = grid_for(c, vector_grid(n));
    bool dist = c->dist;
    // partial-sum slots (vtk_ctx::d_part, GMAX each)
    double *p_vv = c->d_part, *p_rv = p_vv + GMAX, *p_ss = p_vv + 2 * GMAX, *p_tt = p_vv + 3 * GMAX;
    double *p_ts = p_vv + 4 * GMAX, *p_rr = p_vv + 5 * GMAX, *p_rho = p_vv + 6 * GMAX, *p_b = p_vv + 7 * GMAX;
    // across ranks: the all-reduced records (BCG_REC_*) and this rank's sticky failure vote
    double *rec = c->d_scal, *my_vote = &c->d_scal[DC_VOTE + 1];
    Vote vote{c, my_vote};   // a launch of the solve that failed: voted across ranks, returned at once on one
    bool fail_pending = c->tune.fail_step >= 0;
    double n8 = 8.0 * n, b_csr = solver_matrix_bytes(A), b_inv = prec_row_bytes(M, true) * n;   // (tridiagonal blocks: the stored l | m | g)
    BjOp bj = bj_op(M);
    bool fuse = M && c->tune.bcg_fuse && bcg_fusable(bj);
    // work: r (s in place) | rtilde | p | v | t | phat | shat, then the device state
    DBuf work;
    double *r = nullptr, *rtilde = nullptr, *p = nullptr, *v = nullptr, *t = nullptr, *phat = nullptr, *shat = nullptr;
    BicgState *ds = nullptr, *hs = nullptr;
    const int *stop = nullptr;
    const double *vote_of(int rec_off) const { return dist ? rec + rec_off : nullptr; }   // the all-reduced vote of a record
#define BSOFT(x) TRY(vote.launch((x), #x))

    // the ranks leave together after a nonzero vote: this rank's own error, or VTK_ERR_PEER
    int left(const std::string &where) {
        prof_flush(c);
        if (vote.local_rc != VTK_OK) return fail(c, vote.local_rc, vote.local_msg);
        return fail(c, VTK_ERR_PEER, "vtk_bicgstab: a peer rank failed " + where + "; every rank left the solve there");
    }
    // across ranks: dst[0..nq) = this rank's sums of q0 (and q1), dst[nq] = its vote (k_bcg_reduce), summed over
    // the ranks; q0 (q1) then view the sums.  One rank: nothing, the consumers sum the partials
    int gsum(Red &q0, Red *q1, double *dst, const int *stp, int tag) {
        if (!dist) return VTK_OK;
        const int nq = q1 ? 2 : 1;
        { Prof pf(c, "bcg_reduce", tag, 8.0 * (q0.cnt + (q1 ? q1->cnt : 0)));
          BSOFT(launch_bcg_reduce(q0, q1 ? *q1 : none, none, none, nq, my_vote, dst, stp, tag, c->stream)); }
        Prof pf(c, "allreduce", tag, 8.0 * (nq + 1));
        TRY(comm_allreduce(c, dst, nq + 1));
        q0 = Red{dst, 1};
        if (q1) *q1 = Red{dst + 1, 1};
        return VTK_OK;
    }
    // products of the loop: y = A x, part0 = sum y^2, part1 = sum v0 y
    int product(const double *xin, double *y, const double *v0, double *part0, double *part1, int tag, int &cnt) {
        TRY(halo_exchange(A, xin));
        Prof pf(c, "spmv_w", tag, b_csr + 3 * n8);
        const SpmvIn in = lsv_in(spmv_in(A, &A->tiles, xin), A);
        BSOFT(launch_spmv(in, EPI_PREC, y, nullptr, BjOp{}, v0, part0, part1, stop, tag, c->stream));
        cnt = spmv_grid(in);
        return VTK_OK;
    }
    int apply(const double *in, double *out, int tag) {
        Prof pf(c, prec_cls(M), tag, b_inv + 2 * n8);
        return prec_apply(c, M, n, in, out, nullptr, nullptr, nullptr, G, stop, tag, &vote);
    }

    // the work vectors (across ranks a failed allocation is voted into the first all-reduce, which
    // every rank is about to enter), then ||b|| and `x.any()`: the host decisions before the loop
    // (bnrm2 == 0, r = b or b - A x), global across ranks: sum b^2, the flag and the vote travel
    // in one all-reduce
    int norms(double &bnrm2, bool &r_is_b) {
        const int arc = dalloc(c, work, (7 * (size_t)ld + 16) * sizeof(double));
        if (arc != VTK_OK) {
            if (!dist) return arc;
            vote.local_rc = arc;
            vote.local_msg = c->err;
        }
        { Prof pf(c, "dot", -1, n8);
          HIPCHK(c, launch_dot(b, nullptr, n, p_b, G, c->stream)); }
        HIPCHK(c, hipMemsetAsync(&c->d_scal[2], 0, sizeof(double), c->stream));
        { Prof pf(c, "any", -1, n8);
          HIPCHK(c, launch_any_nonzero(x, n, &c->d_scal[2], c->stream)); }
        double h3[3] = {0.0, 0.0, 0.0};
        if (dist) {
            HIPCHK(c, hipMemsetAsync(my_vote, vote.local_rc == VTK_OK ? 0 : 1, sizeof(double), c->stream));
            Red qb{p_b, G}, qx{&c->d_scal[2], 1};
            TRY(gsum(qb, &qx, rec + BCG_REC_PRE, nullptr, -1));
            TRY(read_back(c, h3, rec + BCG_REC_PRE));
            if (h3[2] != 0.0) return left("before the first iteration");
            bnrm2 = std::sqrt(h3[0]);
            r_is_b = h3[1] == 0.0;
        } else {
            HIPCHK(c, launch_finalize(Red{p_b, G}, &c->d_scal[0], 1, c->stream));
            TRY(read_back(c, h3, c->d_scal));
            bnrm2 = h3[0];
            r_is_b = h3[2] == 0.0;
        }
        r = work.as<double>(), rtilde = r + ld, p = rtilde + ld, v = p + ld, t = v + ld;
        phat = M ? t + ld : p, shat = M ? t + 2 * ld : r;   // no preconditioner: M p = p, M s = s
        ds = reinterpret_cast<BicgState *>(r + 7 * (size_t)ld);
        hs = reinterpret_cast<BicgState *>(c->h_state);
        stop = &ds->stop;
        return VTK_OK;
    }

    // r = b - A x if x.any() else b; rtilde = r; the state record; the initial scalar step
    int start(bool r_is_b) {
        Red rr0{p_b, G};
        if (r_is_b) {
            HIPCHK(c, hipMemcpyAsync(r, b, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        } else {
            TRY(halo_exchange(A, x));
            Prof pf(c, "spmv_resid", -1, b_csr + 3 * n8);
            const SpmvIn in = lsv_in(spmv_in(A, &A->tiles, x), A);
            BSOFT(launch_spmv(in, EPI_RESID, r, b, BjOp{}, nullptr, p_rr, nullptr, nullptr, 0, c->stream));
            rr0 = Red{p_rr, spmv_grid(in)};
        }
        HIPCHK(c, hipMemcpyAsync(rtilde, r, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        std::memset(hs, 0, sizeof(BicgState));
        hs->stop = BCG_RUN;
        HIPCHK(c, hipMemcpyAsync(ds, hs, sizeof(BicgState), hipMemcpyHostToDevice, c->stream));
        *c->h_stop = BCG_RUN;
        TRY(gsum(rr0, nullptr, rec + BCG_REC_INIT, stop, 0));   // the initial residual's partials, summed over the ranks
        Prof pf(c, "bcg_scalar", 0, 8.0 * rr0.cnt);
        BSOFT(launch_bcg_scalar(BCG_PH_INIT, 0, 0, info_max, atol, rr0, none, none, none, vote_of(BCG_REC_INIT + 1), ds, c->d_stop, stop, 0, c->stream));
        return VTK_OK;
    }

    // Iteration k.  Across ranks every sum a scalar step or k_bcg_x consumes is all-reduced first
    // (four collectives per iteration: A, B, omega, C), each record carrying the vote; every rank
    // then reads the same bits and computes the same alpha, omega, beta and the same stop
    int iteration(int64_t k, bool last) {
        const int t1 = bcg_tag(k, 1), t3 = bcg_tag(k, 3);
        const int first = k == 0 ? 1 : 0;
        int cnt = 0;
        bool refused = false;
        if (fail_pending && k == c->tune.fail_step) {   // test hook: as if this iteration's first launch were refused
            fail_pending = false;
            refused = true;
            TRY(vote.launch(hipErrorLaunchFailure, "injected failure (tuning fail_step)"));
        }
        // p = r + beta (p - omega v); phat = M p; v = A phat; rv = <rtilde, v>; alpha
        if (!refused) {
            Prof pf(c, "bcg_p", t1, (first ? 2 : 4) * n8 + (fuse ? b_inv + n8 : 0.0));
            BSOFT(launch_bcg_p(ds, first, n, r, v, p, fuse ? &bj : nullptr, phat, G, stop, t1, c->stream));
        }
        if (M && !fuse) TRY(apply(p, phat, t1));
        TRY(product(phat, v, rtilde, p_vv, p_rv, t1, cnt));
        Red q_rv{p_rv, cnt};
        TRY(gsum(q_rv, nullptr, rec + BCG_REC_A, stop, t1));
        { Prof pf(c, "bcg_scalar", t1, 8.0 * q_rv.cnt);
          BSOFT(launch_bcg_scalar(BCG_PH_A, k, 0, info_max, atol, none, q_rv, none, none, vote_of(BCG_REC_A + 1), ds, c->d_stop, stop, t1, c->stream)); }
        // s = r - alpha v (in r); ||s|| < atol: the half-step exit
        { Prof pf(c, "bcg_s", t1, 3 * n8 + (fuse ? b_inv + n8 : 0.0));
          BSOFT(launch_bcg_s(ds, n, r, v, fuse ? &bj : nullptr, shat, p_ss, G, stop, t1, c->stream)); }
        Red q_ss{p_ss, G};
        TRY(gsum(q_ss, nullptr, rec + BCG_REC_B, stop, t1));
        { Prof pf(c, "bcg_scalar", t1, 8.0 * q_ss.cnt);
          BSOFT(launch_bcg_scalar(BCG_PH_B, k, 0, info_max, atol, q_ss, none, none, none, vote_of(BCG_REC_B + 1), ds, c->d_stop, stop, t1, c->stream)); }
        // shat = M s; t = A shat; omega = <t, s> / <t, t>; x += alpha phat + omega shat; r = s - omega t
        if (M && !fuse) TRY(apply(r, shat, t3));
        TRY(product(shat, t, r, p_tt, p_ts, t3, cnt));
        Red q_ts{p_ts, cnt}, q_tt{p_tt, cnt}, q_rr{p_rr, G}, q_rho{p_rho, G};
        TRY(gsum(q_ts, &q_tt, rec + BCG_REC_W, stop, t3));
        { Prof pf(c, "bcg_x", t3, 8 * n8 + 8.0 * (q_ts.cnt + q_tt.cnt));
          BSOFT(launch_bcg_x(ds, q_ts, q_tt, n, x, phat, shat, r, t, rtilde, p_rr, p_rho, vote_of(BCG_REC_W + 2), G, stop, t3, c->stream)); }
        TRY(gsum(q_rr, &q_rho, rec + BCG_REC_C, stop, t3));
        Prof pf(c, "bcg_scalar", t3, 8.0 * (q_ts.cnt + q_tt.cnt + q_rr.cnt + q_rho.cnt));
        BSOFT(launch_bcg_scalar(BCG_PH_C, k, last ? 1 : 0, info_max, atol, q_ts, q_tt, q_rr, q_rho, vote_of(BCG_REC_C + 2), ds, c->d_stop, stop, t3, c->stream));
        return VTK_OK;
    }

    // after the loop: the stop record, the half-step x update, the true residual of the returned x
    // (t is free now); across ranks its all-reduce carries the last vote: a failure after the stop
    // record still reaches every rank
    int finish(double &rnorm) {
        TRY(read_back(c, *hs, ds));
        if (hs->stop == BCG_RUN) {   // (across ranks: voted into the last all-reduce, which the peers enter)
            if (!dist) return fail(c, VTK_ERR_HIP, "vtk_bicgstab: the loop ended without a stop record");
            TRY(vote.launch(hipErrorLaunchFailure, "vtk_bicgstab: the loop ended without a stop record"));
        }
        const int64_t its = hs->iterations;
        if (hs->half_step) {   // x += alpha phat: the flag sits at that iteration's half-step tag
            Prof pf(c, "bcg_x", -1, 3 * n8);
            BSOFT(launch_bcg_half_x(ds, n, x, phat, G, stop, bcg_tag(its - 1, 2), c->stream));
        }
        TRY(halo_exchange(A, x));
        const SpmvIn in = lsv_in(spmv_in(A, &A->tiles, x), A);
        { Prof pf(c, "spmv_resid", -1, b_csr + 3 * n8);
          BSOFT(launch_spmv(in, EPI_RESID, t, b, BjOp{}, nullptr, p_rr, nullptr, nullptr, 0, c->stream)); }
        if (dist) {
            double h2[2] = {0.0, 0.0};
            Red q_fin{p_rr, spmv_grid(in)};
            TRY(gsum(q_fin, nullptr, rec + BCG_REC_FIN, nullptr, -1));
            TRY(read_back(c, h2, rec + BCG_REC_FIN));
            if (h2[1] != 0.0)
                return left(hs->peer_failed ? "in iteration " + std::to_string(its) : std::string("after the last iteration"));
            rnorm = std::sqrt(h2[0]);
        } else {
            HIPCHK(c, launch_finalize(Red{p_rr, spmv_grid(in)}, &c->d_scal[1], 1, c->stream));
            TRY(read_back(c, rnorm, &c->d_scal[1]));
        }
        return VTK_OK;
    }
#undef BSOFT
};

}  // namespace

int vtk::run_bicgstab(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol, int64_t maxiter,
                      int *info, vtk_bicgstab_stats *stout) {
    vtk_ctx *c = A->ctx;
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = A->n_local, N = A->n_global;
    if (N < 1) return fail(c, VTK_ERR_ARG, "vtk_bicgstab: empty system");
    if (maxiter <= 0) maxiter = N * 10;                     // iterative.py: maxiter None -> n * 10
    const int info_max = (int)std::min<int64_t>(maxiter, INT32_MAX);
    maxiter = std::min(maxiter, BCG_MAX_ITERS);
    Bicg s{A, M, c, b, x, info_max};
    double bnrm2 = 0.0;
    bool r_is_b = true;
    TRY(s.norms(bnrm2, r_is_b));
    s.atol = atol = std::max(atol, rtol * bnrm2);           // _get_atol_rtol
    vtk_bicgstab_stats st{};
    st.bnorm = bnrm2;
    st.atol_eff = atol;
    if (bnrm2 == 0.0) {                                     // return postprocess(b), 0
        HIPCHK(c, hipMemcpyAsync(x, b, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        prof_flush(c);
        return solve_done(info, 0, st, stout, t0);
    }
    TRY(s.start(r_is_b));
    EvRing ev;
    TRY(ev.create(c));
    volatile int *mirror = c->h_stop;
    for (int64_t k = 0; k < maxiter; ++k) {
        TRY(s.iteration(k, k + 1 == maxiter));
        HIPCHK(c, hipEventRecord(ev.e[k % (LOOKAHEAD + 1)], c->stream));
        if (k >= LOOKAHEAD) {
            HIPCHK(c, hipEventSynchronize(ev.e[(k - LOOKAHEAD) % (LOOKAHEAD + 1)]));
            // across ranks the test is a function of device state alone (the GMRES loop's comparison):
            // a stop of an iteration up to k - LOOKAHEAD, so every rank enqueues the same iterations
            // and the same collectives; one rank: whatever the mirror shows by now
            if (s.dist ? *mirror <= bcg_tag(k - LOOKAHEAD, 3) : *mirror != BCG_RUN) break;
        }
    }
    TRY(s.finish(st.rnorm));
    if (c->prof_on) prof_flush(c, s.hs->stop);
    st.iterations = s.hs->iterations;
    st.half_step = s.hs->half_step;
    // algorithmic bytes: per iteration two products, two applies, p (4 vectors), s (3), x (8)
    const double per_it = 2 * (s.b_csr + 3 * s.n8) + (M ? 2 * (s.b_inv + 2 * s.n8) : 0.0) + 15 * s.n8;
    st.bytes_moved = per_it * (double)s.hs->iterations + 2 * (s.b_csr + 3 * s.n8) + 4 * s.n8;
    return solve_done(info, s.hs->info, st, stout, t0);
}
