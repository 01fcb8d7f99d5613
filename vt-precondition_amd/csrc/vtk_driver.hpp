// vtk_driver.hpp -- what the host units of libvtkrylov.so share (vtk_api.cpp, vtk_operator.cpp,
// vtk_precond.cpp, vtk_apply.cpp, vtk_gmres.cpp, vtk_bicg.cpp): error returns, scope-owned device
// buffers, the kernel profile, the communicator primitives, the SpMV launch inputs and the operator's
// byte models; then each unit's entry points.  Host only: never included from a .hip file.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "vtk_internal.hpp"

namespace vtk {

std::string context_free_error();   // vtk_host.cpp

constexpr int LOOKAHEAD = 3;   // columns the host may run ahead of the device

inline int fail(vtk_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    else set_context_free_error(msg);
    return code;
}

#define HIPCHK(c, x)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (x);                                                                 \
        if (e_ != hipSuccess)                                                                \
            return fail((c), e_ == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP,        \
                        std::string(#x) + ": " + hipGetErrorString(e_));                     \
    } while (0)

#define NCCLCHK(c, x)                                                                        \
    do {                                                                                     \
        ncclResult_t r_ = (x);                                                               \
        if (r_ != ncclSuccess) {                                                             \
            if (c) (c)->comm_broken = true;                                                  \
            return fail((c), VTK_ERR_RCCL, std::string(#x) + ": " + ncclGetErrorString(r_)); \
        }                                                                                    \
    } while (0)

#define TRY(x)                          \
    do {                                \
        int rc_ = (x);                  \
        if (rc_ != VTK_OK) return rc_;  \
    } while (0)

// device buffer owned by a scope
struct DBuf {
    void *p = nullptr;
    ~DBuf() { if (p) (void)hipFree(p); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

inline int dalloc(vtk_ctx *c, DBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    HIPCHK(c, hipMalloc(&b.p, bytes));
    return VTK_OK;
}

// a small device record on the host, once the stream has finished
template <typename T>
int read_back(vtk_ctx *c, T &h, const void *d) {
    HIPCHK(c, hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

inline int64_t round_up(int64_t a, int64_t m) { return (a + m - 1) / m * m; }

// ---- kernel profile: HIP events around each launch on the context stream ------------------
inline hipEvent_t prof_event(vtk_ctx *c) {
    if (!c->prof_pool.empty()) { hipEvent_t e = c->prof_pool.back(); c->prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

inline int prof_class(vtk_ctx *c, const char *name) {
    for (size_t i = 0; i < c->prof_acc.size(); ++i) if (c->prof_acc[i].name == name) return (int)i;
    c->prof_acc.push_back(vtk_ctx::ProfAcc{name});
    return (int)c->prof_acc.size() - 1;
}

// brackets one launch: start event at construction, stop event at scope exit
struct Prof {
    vtk_ctx *c;
    size_t idx = (size_t)-1;
    Prof(vtk_ctx *c_, const char *name, int col, double bytes) : c(c_) {
        if (!c->prof_on || !name) return;   // (no class name: the caller brackets the launch itself)
        vtk_ctx::ProfPending p{prof_class(c, name), col, bytes, prof_event(c), prof_event(c)};
        (void)hipEventRecord(p.e0, c->stream);
        c->prof_pending.push_back(p);
        idx = c->prof_pending.size() - 1;
    }
    ~Prof() { if (idx != (size_t)-1) (void)hipEventRecord(c->prof_pending[idx].e1, c->stream); }
};

// fold pending launches into the per-class counters; launches of columns after the cycle's
// stop column (no-op kernels) are dropped
inline void prof_flush(vtk_ctx *c, int last_col = 1 << 30) {
    if (c->prof_pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto &p : c->prof_pending) {
        if (p.col <= last_col) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
                auto &a = c->prof_acc[p.cls];
                a.launches += 1;
                a.seconds += ms * 1e-3;
                a.bytes += p.bytes;
            }
        }
        c->prof_pool.push_back(p.e0);
        c->prof_pool.push_back(p.e1);
    }
    c->prof_pending.clear();
}

// the BJ operator the kernels apply (vtk_bj_mode): tridiagonal factors when available and not
// switched off, else the inverse rows; null M, or any other kind: the empty BjOp (identity) -- only
// block Jacobi has an epilogue form (bj_fused, bj8_tri and bcg_fusable guard its consumers; the other
// kinds apply through kind_apply, vtk_apply.cpp)
inline BjOp bj_op(const vtk_prec *M) {
    BjOp o;
    if (!M || M->kind != VTK_PREC_BJACOBI) return o;
    o.inv = M->d_inv;
    o.bs = M->bs;
    // a lagged M (not refreshed since its operator's last value update, vtk_prec_refresh) applies
    // its inverse rows: the SELL kernels' tridiagonal apply reads only m of M's factors and takes
    // the blocks' sub- and super-diagonals from the operator's rows -- those are A's new values
    // now, not the ones M was factored from, and the mix is no preconditioner at all (C0 with
    // lagged factors: no convergence).  The inverse rows are M's own data throughout.
    if (M->tri_ok && M->mode != VTK_BJ_INVERSE && M->epoch == M->A->values_epoch) {
        o.tri = M->d_tri;
        o.tri_ld = M->tri_ld;
    }
    return o;
}

// tridiagonal BJ(8) with current factors: what the band step, the x-line ring and the 4D ring
// apply (their m tables are M's factors; a lagged M has none, bj_op)
inline bool bj8_tri(const vtk_prec *M) {
    return M && M->kind == VTK_PREC_BJACOBI && M->bs == 8 && bj_op(M).tri != nullptr;
}

inline bool bj_fused(const vtk_prec *M);

// the Neumann wrapper's corrections run in one SpMV launch each (EPI_NEU_CORR): a base with
// BJ-fused tiles, bs <= 8 (tuning neu_fuse 0: the three-launch form, the same bits)
inline bool neu_fused(const vtk_prec *N) {
    return N && N->kind == VTK_PREC_NEUMANN && N->A->ctx->tune.neu_fuse && bj_fused(N->base) && N->base->bs <= 8;
}

// reducing-kernel grid: a function of the local size on one GPU; GMAX on every rank when
// world > 1 (equal partial-vector lengths for the in-place all-reduce; vtk_gmres.cpp residual()
// relies on it: its shared tail's pad_partials must find the SpMV launches' partials at full length)
inline int grid_for(vtk_ctx *c, int g) { return c->dist ? GMAX : g; }

// Bytes of the operator one SpMV reads in the layout in use (the algorithmic figure of the
// profile classes): CSR = values + int32 columns + indptr; SELL = values
// (padding included) + offsets, + int32 columns, or (dictionary-coded) 4-bit codes + 64-B
// dictionaries + the wide chunks' int32 columns.
inline double matrix_bytes(const vtk_csr *A) {
    const double vb = A->fp32 ? 4.0 : 8.0;
    if (!A->use_sell) return (vb + 4.0) * A->nnz + 4.0 * (A->n_local + 1);
    const Sell &sl = A->sell;
    double b = vb * sl.entries + 8.0 * (sl.nch + 1);
    if (sl.d_pk) b += 4.0 * sl.pk_words + 72.0 * sl.nch + 4.0 * sl.wide_entries;
    else b += 4.0 * sl.entries;
    return b;
}

// ---- communicator primitives: RCCL on the context stream, or host-staged hooks ------------

// in-place sum over ranks of `count` doubles in device memory
inline int comm_allreduce(vtk_ctx *c, double *d, int64_t count) {
    if (c->host_comm) {
        std::vector<double> h((size_t)count);
        HIPCHK(c, hipMemcpyAsync(h.data(), d, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->hops.allreduce_sum_f64(c->hops.user, h.data(), count) != 0) return fail(c, VTK_ERR_STATE, "host allreduce hook failed");
        HIPCHK(c, hipMemcpyAsync(d, h.data(), count * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VTK_OK;
    }
    NCCLCHK(c, ncclAllReduce(d, d, (size_t)count, ncclDouble, ncclSum, c->comm, c->stream));
    return VTK_OK;
}

// point-to-point exchange: to rank q scnt[q] elements from send+soff[q], from rank q rcnt[q]
// elements into recv+roff[q] (ncclSend/ncclRecv in one group: xGMI is point-to-point)
inline int comm_alltoallv(vtk_ctx *c, const void *send, const std::vector<int64_t> &scnt, const std::vector<int64_t> &soff,
                   void *recv, const std::vector<int64_t> &rcnt, const std::vector<int64_t> &roff, ncclDataType_t dt, size_t eb,
                   hipStream_t st = nullptr) {
    const int W = c->world;
    if (!st) st = c->stream;
    if (c->host_comm) {
        const int64_t ns = W ? soff[W - 1] + scnt[W - 1] : 0, nr = W ? roff[W - 1] + rcnt[W - 1] : 0;
        std::vector<char> hs((size_t)std::max<int64_t>(ns, 1) * eb), hr((size_t)std::max<int64_t>(nr, 1) * eb);
        if (ns) HIPCHK(c, hipMemcpyAsync(hs.data(), send, ns * eb, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (c->hops.alltoallv(c->hops.user, hs.data(), scnt.data(), soff.data(), hr.data(), rcnt.data(), roff.data(), (int64_t)eb) != 0)
            return fail(c, VTK_ERR_STATE, "host alltoallv hook failed");
        if (nr) HIPCHK(c, hipMemcpyAsync(recv, hr.data(), nr * eb, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
        return VTK_OK;
    }
    NCCLCHK(c, ncclGroupStart());
    for (int q = 0; q < W; ++q) {
        if (scnt[q] > 0) NCCLCHK(c, ncclSend((const char *)send + soff[q] * eb, (size_t)scnt[q], dt, q, c->comm, st));
        if (rcnt[q] > 0) NCCLCHK(c, ncclRecv((char *)recv + roff[q] * eb, (size_t)rcnt[q], dt, q, c->comm, st));
    }
    NCCLCHK(c, ncclGroupEnd());
    return VTK_OK;
}

// every rank contributes `count` int64 (device), receives world*count (device)
inline int comm_allgather_i64(vtk_ctx *c, const int64_t *send, int64_t *recv, int64_t count) {
    if (c->host_comm) {
        std::vector<int64_t> hs((size_t)count), hr((size_t)count * c->world);
        HIPCHK(c, hipMemcpyAsync(hs.data(), send, count * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->hops.allgather(c->hops.user, hs.data(), hr.data(), count * 8) != 0) return fail(c, VTK_ERR_STATE, "host allgather hook failed");
        HIPCHK(c, hipMemcpyAsync(recv, hr.data(), hr.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VTK_OK;
    }
    NCCLCHK(c, ncclAllGather(send, recv, (size_t)count, ncclInt64, c->comm, c->stream));
    return VTK_OK;
}

// every rank contributes `count` doubles (device), receives world*count (device); one rank without
// a communicator: a device copy
inline int comm_allgather(vtk_ctx *c, const double *send, double *recv, int64_t count) {
    if (!c->dist) {
        HIPCHK(c, hipMemcpyAsync(recv, send, (size_t)count * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        return VTK_OK;
    }
    if (c->host_comm) {
        std::vector<double> hs((size_t)count), hr((size_t)count * c->world);
        HIPCHK(c, hipMemcpyAsync(hs.data(), send, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->hops.allgather(c->hops.user, hs.data(), hr.data(), count * (int64_t)sizeof(double)) != 0)
            return fail(c, VTK_ERR_STATE, "host allgather hook failed");
        HIPCHK(c, hipMemcpyAsync(recv, hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return VTK_OK;
    }
    NCCLCHK(c, ncclAllGather(send, recv, (size_t)count, ncclDouble, c->comm, c->stream));
    return VTK_OK;
}

// partial sums -> consumer view.  Across ranks every reducing kernel runs on exactly GMAX
// workgroups (grid_for), so the partial vectors have the same length on every rank and are
// all-reduced in place: consumers then sum them exactly as on one GPU, with no extra kernel.
inline int reduce(vtk_ctx *c, double *part, int cnt, Red &out) {
    out = Red{part, cnt};
    if (!c->dist) return VTK_OK;
    Prof pf(c, "allreduce", -1, 8.0 * cnt);
    return comm_allreduce(c, part, cnt);
}

// across ranks the all-reduced partial vectors must have one length on every rank: a reducing
// launch whose grid follows the slab (the 4D and x-line rings) zero-pads its partials to GMAX, as
// every other reducing launch runs GMAX workgroups there (grid_for)
inline int pad_partials(vtk_ctx *c, double *p0, double *p1, int &g) {
    if (!c->dist || g >= GMAX) return VTK_OK;
    for (double *p : {p0, p1})
        if (p) HIPCHK(c, hipMemsetAsync(p + g, 0, (size_t)(GMAX - g) * sizeof(double), c->stream));
    g = GMAX;
    return VTK_OK;
}

inline int halo_exchange(vtk_csr *A, const double *x) {
    vtk_ctx *c = A->ctx;
    // no peer of this rank: RCCL point-to-point needs no call; the host-staged alltoallv is a
    // collective every rank joins (with zero counts)
    if (!c->dist || (!c->host_comm && A->n_send == 0 && A->n_halo == 0)) return VTK_OK;
    Prof pf(c, "halo", -1, 16.0 * A->n_send + 8.0 * A->n_halo);
    HIPCHK(c, launch_gather(x, A->d_send_idx, A->n_send, A->d_send_buf, c->stream));
    return comm_alltoallv(c, A->d_send_buf, A->send_cnt, A->send_off, A->d_halo, A->recv_cnt, A->recv_off, ncclDouble, sizeof(double));
}

// the same exchange overlapped: pack and send/recv both on the comm stream once x is final on
// the main stream (ev_pack); the interior tiles start at once, ev_halo marks the halo's arrival
// (the boundary tiles wait on it)
inline int halo_exchange_async(vtk_csr *A, const double *x) {
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipEventRecord(c->ev_pack, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_pack, 0));
    HIPCHK(c, launch_gather(x, A->d_send_idx, A->n_send, A->d_send_buf, c->comm_stream));
    TRY(comm_alltoallv(c, A->d_send_buf, A->send_cnt, A->send_off, A->d_halo, A->recv_cnt, A->recv_off, ncclDouble,
                       sizeof(double), c->comm_stream));
    HIPCHK(c, hipEventRecord(c->ev_halo, c->comm_stream));
    return VTK_OK;
}

inline SpmvIn spmv_in(vtk_csr *A, const Tiles *t, const double *x, const Groups *g = nullptr) {
    SpmvIn in{A->d_indptr, A->d_indices, A->d_data, A->fp32, t, (int)A->n_local, x,
              A->ctx->dist ? A->d_halo : nullptr};
    if (A->use_sell) {   // SELL-64 layout: the tiles are not used
        in.sell = &A->sell;
        in.groups = g ? g : &A->g_all;
    }
    in.plain_grid = 2048;   // (grid sweep, C3: 2048 best; 3072: 293 us; 4096-100 000: 256-265)
    // the plain SpMV walks its groups in XCD-contiguous order (C3 PMC fetch 1.40 -> 1.07 GB per
    // launch, time neutral) -- except on the 9-wide 4D rows (648 -> 730 us swizzled: their x +- 1
    // planes are 250 000 rows away, not in the XCD's window); the reducing launches keep
    // blockIdx order, so their partial sums keep their bits
    in.swz = (A->use_sell && A->sell.uniform_w > 8) ? 0 : 1;
    in.plain_var = 1;   // padding gathers branched in the plain SpMV (243.6 -> 221.3 us)
    return in;
}

// the fused SpMV + BJ kernels apply: SELL chunks align with any power-of-two bs <= 32; the
// CSR-stream path needs the BJ tiles aligned and free of long rows
inline bool bj_fused(const vtk_prec *M) {
    if (!M || M->kind != VTK_PREC_BJACOBI) return false;
    if (M->A->use_sell) return (M->bs & (M->bs - 1)) == 0 && M->bs <= 32;
    return M->fused;
}

// the solver's SELL launches read the line-separable tables when the operator
// has them: the same values, the same sums, 8 B of values per row instead of 40 (tuning band_lsv
// 0: the SELL values).  vtk_spmv keeps the SELL values: it is the measured SpMV
inline bool lsv_on(const vtk_csr *A) {
    return A->use_sell && A->d_lsv && A->band_L > 0 && !A->fp32 && A->ctx->tune.band_lsv &&
           (!A->ctx->dist || A->band_ghost);
}
inline SpmvIn lsv_in(SpmvIn in, const vtk_csr *A) {
    if (in.sell && A->d_g4tab && A->ctx->tune.grid4) in.g4 = A->g4;   // 4D grid rows (Grid4)
    if (in.sell && lsv_on(A)) {
        in.lsv = A->d_lsv;
        in.lsv_L = (int)A->band_L;
        in.lsv_lblk = A->band_ghost ? A->band_lblk : -1;
        in.lsv_xord = A->band_ghost ? A->band_xord : 0;
        // tuning sell_canon 0 (A/B): the SELL codes even for canonical rows
        in.lsv_canon = A->lsv_canon && A->ctx->tune.sell_canon ? 1 : 0;
    }
    return in;
}
// matrix bytes a solver SELL launch reads (lsv_in)
inline double solver_matrix_bytes(const vtk_csr *A) {
    const double b = matrix_bytes(A);
    if (A->use_sell && A->d_g4tab && A->ctx->tune.grid4) return (A->fp32 ? 4.0 : 8.0) * (double)A->n_local;   // D only
    if (!lsv_on(A)) return b;
    if (A->lsv_canon && A->ctx->tune.sell_canon) return 8.0 * (double)A->n_local;   // the diagonal only
    return b - 8.0 * (double)A->sell.entries + 8.0 * (double)A->n_local;
}

// interior / boundary pieces of the fused SpMV (world > 1)
inline bool bj_split(const vtk_prec *M) { return M && (M->A->use_sell ? M->A->g_in.grid > 0 : M->split); }
inline SpmvIn split_in(vtk_csr *A, vtk_prec *M, const double *x, bool interior) {
    return lsv_in(interior ? spmv_in(A, &M->tiles_in, x, &A->g_in) : spmv_in(A, &M->tiles_bd, x, &A->g_bd), A);
}

// A launch of a solve that failed.  On one rank: the error returns at once.  Across ranks the
// peers are already inside this step's collectives, so returning would leave them blocked: the
// rank records its error, sets its failure vote (*addr = d_scal[DC_VOTE + 1], summed into the next
// all-reduce by k_dc_finalize / k_bcg_reduce) and goes on issuing the same launches and
// collectives; the vote stops every rank at the same point and the solver returns the error there
// (VTK_ERR_PEER on the other ranks).  (Pattern: the reference's step runner turns a step's
// exception into a return code, precondition_setup/vtsetup/vt_precondition.py:66-79.)
struct Vote {
    vtk_ctx *c;
    double *addr;
    int local_rc = VTK_OK;    // the first failure of this rank
    std::string local_msg;
    int launch(hipError_t e, const char *what) {
        if (e == hipSuccess) return VTK_OK;
        const int code = e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP;
        const std::string msg = std::string(what) + ": " + hipGetErrorString(e);
        if (!c->dist) return fail(c, code, msg);
        if (local_rc == VTK_OK) {
            local_msg = msg + " (the ranks left the solve together at the next all-reduce)";
            local_rc = fail(c, code, local_msg);
            HIPCHK(c, hipMemsetAsync(addr, 1, sizeof(double), c->stream));
        }
        return VTK_OK;
    }
};

// a launch that may be refused: voted when there is a vote (inside a solve), else it fails at once
inline int soft_launch(vtk_ctx *c, Vote *vote, hipError_t e, const char *what) {
    if (vote) return vote->launch(e, what);
    if (e == hipSuccess) return VTK_OK;
    return fail(c, e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define SOFT_LAUNCH(c, vote, x) TRY(soft_launch((c), (vote), (x), #x))

// the throttle events of a solve (the host runs LOOKAHEAD steps ahead of the device)
struct EvRing {
    hipEvent_t e[LOOKAHEAD + 1] = {};
    int create(vtk_ctx *c) {
        for (auto &v : e) HIPCHK(c, hipEventCreateWithFlags(&v, hipEventDisableTiming));
        return VTK_OK;
    }
    ~EvRing() { for (auto v : e) if (v) (void)hipEventDestroy(v); }
};

// a solve's normal return: info, the elapsed time, the stats record
template <typename Stats>
int solve_done(int *info, int inf, Stats &st, Stats *stout, std::chrono::steady_clock::time_point t0) {
    *info = inf;
    st.t_solve = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (stout) *stout = st;
    return VTK_OK;
}

// ---- vtk_operator.cpp: layout and setup of a vtk_csr ------------------------------------------
int upload_tiles(vtk_ctx *c, const std::vector<int32_t> &indptr, int align, Tiles &t,
                 std::vector<int32_t> *rows_out = nullptr);
void free_tiles(Tiles &t);
int upload_split_tiles(vtk_ctx *c, const std::vector<int32_t> &rows, const std::vector<uint8_t> &row_halo,
                       const Tiles &all, Tiles &in, Tiles &bd);
int apply_layout(vtk_csr *A, int layout);
int finish_csr(vtk_csr *A);
int check_partition(vtk_ctx *c, int64_t n_global, const int64_t *offsets, std::vector<int64_t> &out);
void destroy_csr(vtk_csr *A);
int band_check_all(vtk_csr *A, int64_t L);
int grid4_set(vtk_csr *A, int64_t Ny, int64_t Nvx, int64_t Nvy);
void set_grid4_tables(vtk_csr *A, Grid4 g, DBuf *tab, DBuf *D);
int auto_grid4(vtk_csr *A);
int auto_line_band(vtk_csr *A);
struct UpdateScratch {
    DBuf lsv, g4tab, g4D, bad;   // bad[0]: the line values' flags, bad[1]: the 4D grid's
    bool want_lsv = false, want_g4 = false;
};
int update_prepare(vtk_csr *A, UpdateScratch &u);
int update_finish(vtk_csr *A, UpdateScratch &u);

// ---- vtk_precond.cpp: factors from the operator's current values, the plans, the registry ------
// the registry of live preconditioners: a Neumann wrapper borrows its base and finds out here
// whether the base still exists (vtk_prec_destroy removes it)
void prec_register(vtk_prec *M);
void prec_unregister(const vtk_prec *M);
bool prec_alive(const vtk_prec *M, uint64_t id);
int bj_factor(vtk_prec *M);
int line_factor(vtk_prec *M);
int line2_factor(vtk_prec *M);
int linec_plan(vtk_prec *M, int64_t stride, int64_t period, int64_t seg);
int linec_span_plan(vtk_prec *M, int64_t stride, int64_t period, int64_t seg);   // collective
int linec_factor(vtk_prec *M);
void linec_free(LineC &C);
int prec_usable(const vtk_prec *M, const char *who);

// ---- vtk_apply.cpp: z = M^-1 r, its profile classes and byte models -----------------------------
// profile class of a standalone apply (null for the Neumann wrapper, which brackets its own launches:
// a null name brackets nothing), and its algorithmic bytes per row less the r read and z written.
// tri_stored: tridiagonal BJ blocks as the stored l | m | g (the standalone apply, the fused BiCGStab
// kernels) where the default counts the SELL epilogue's m alone
const char *prec_cls(const vtk_prec *M);
double prec_row_bytes(const vtk_prec *M, bool tri_stored = false);
// DCGS2 step j's operands, for an apply that ends the step's operator: where the kind's last kernel
// has a dots form it writes the dots partials in launch_dc_dots' layout
struct StepDots {
    const double *V;
    int64_t ld;
    int j;
    double *part;
};
// one apply of a non-wrapper kind (kind_apply): z = M^-1 r, or acc + M^-1 r (the kernels' zadd; z must
// not alias acc).  part0 = sum z^2, part1 = sum v0 z over `grid` workgroups (optional), of the last write
struct Apply {
    const double *r;
    double *z;
    const double *acc = nullptr;
    const double *v0 = nullptr;
    double *part0 = nullptr, *part1 = nullptr;
    int grid = 0;
    const int *stop = nullptr;
    int col = 0;
    Vote *vote = nullptr;             // a refused launch is voted (a solve); null: it fails at once
    const StepDots *dots = nullptr;   // asked for: *cnt = grid where the last kernel wrote them, else 0
    bool prof = false;                // each launch under its own class; false: the caller brackets the apply
    const char *last_cls = nullptr;   // prof: the last launch's class when not the kind's own ("neu_corr")
    bool chunk = false;               // lines that span the ranks: the rank's chunk alone (their factorisation)
};
// the launches of kind M->kind (null M: the identity), each kind's sequence once
int kind_apply(vtk_ctx *c, vtk_prec *M, int64_t n, const Apply &a, int *cnt = nullptr);
// z = M^-1 r for every kind: kind_apply, or the Neumann wrapper's corrections around it (each with its
// halo exchange; dots and cnt reach the wrapper only).  r and z must not alias for the wrapper
int prec_apply(vtk_ctx *c, vtk_prec *M, int64_t n, const double *r, double *z, const double *v0, double *part0,
               double *part1, int grid, const int *stop_col, int col, Vote *vote, const StepDots *dots = nullptr,
               int *cnt = nullptr);

// ---- vtk_gmres.cpp / vtk_bicg.cpp: the drivers, and the step launches vtk_precond_matvec shares -
int run_gmres(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
              int restart, int64_t maxiter, int *info, vtk_stats *stout);
int run_bicgstab(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol, int64_t maxiter,
                 int *info, vtk_bicgstab_stats *stout);
bool g4_ring_ok(vtk_ctx *c, const vtk_csr *A, const vtk_prec *M);
bool line_fuse_ok(vtk_ctx *c, const vtk_csr *A, const vtk_prec *M);
int g4_ring_split(vtk_csr *A, const vtk_prec *M, const double *x, double *w, bool exch, Vote *vote, const char *cls,
                  double bytes, const G4Dots *dots, const int *stop, int col, int *cnt);

}  // namespace vtk
