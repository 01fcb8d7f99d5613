// vtk_api.cpp -- C-ABI of libvtkrylov.so: argument checks, contexts, the RCCL / host-staged
// communicator, the tuning switches, and the entry points that hand over to the other host units
// (vtk_operator.cpp, vtk_precond.cpp, vtk_apply.cpp, vtk_gmres.cpp, vtk_bicg.cpp; shared pieces:
// vtk_driver.hpp).
#include <cctype>
#include <climits>
#include <cstdlib>

#include "vtk_driver.hpp"
#include "vtk_vlasov.hpp"

namespace vtk {
bool vlasov_params_ok(const vtk_vlasov_params *p);
}  // namespace vtk

using namespace vtk;

namespace {

// ---- tuning switches (vtk::Tuning): name, member; VTK_<NAME upper> seeds them at creation ----
struct TuneKey { const char *name; int Tuning::*mem; };
constexpr TuneKey TUNE_KEYS[] = {
    {"band", &Tuning::band}, {"band_lsv", &Tuning::band_lsv}, {"sell_canon", &Tuning::sell_canon},
    {"band_canon", &Tuning::band_canon}, {"band_opt", &Tuning::band_opt}, {"band_long_rows", &Tuning::band_long_rows},
    {"lsv_ring", &Tuning::lsv_ring},
    {"prof_perj", &Tuning::prof_perj}, {"comm_solo", &Tuning::comm_solo}, {"auto_band", &Tuning::auto_band},
    {"grid4", &Tuning::grid4}, {"c4_fused", &Tuning::c4_fused}, {"g4_ring", &Tuning::g4_ring},
    {"g4_gr", &Tuning::g4_gr}, {"g4_fast", &Tuning::g4_fast}, {"line_fuse", &Tuning::line_fuse}, {"cyc_ring", &Tuning::cyc_ring},
    {"line2_dc", &Tuning::line2_dc}, {"linec_serial", &Tuning::linec_serial},
    {"bcg_fuse", &Tuning::bcg_fuse}, {"neu_fuse", &Tuning::neu_fuse}, {"neu_dc", &Tuning::neu_dc},
    {"fail_step", &Tuning::fail_step},
};
// switches of earlier rounds whose alternative lost its A/B: an environment that
// still sets one is told once that it no longer has an effect
constexpr const char *RETIRED_KEYS[] = {"band_canon_sl", "sell_pad", "sell_grid", "plain_grid", "sell_swz", "plain_var",
                                        "band_j3", "lsv_spmv_cap", "line_sweep", "ev_every", "debug_band", "g4_pd",
                                        "g4_xcd", "g4_dc", "g4_dc0", "g4_res", "upd_grid", "upd_xb", "sell_nopad",
                                        "sell_lsv"};

const TuneKey *tune_key(const char *name) {
    if (!name) return nullptr;
    for (const auto &k : TUNE_KEYS)
        if (std::strcmp(k.name, name) == 0) return &k;
    return nullptr;
}

std::string env_name(const char *key) {
    std::string var = "VTK_";
    for (const char *p = key; *p; ++p) var += (char)std::toupper((unsigned char)*p);
    return var;
}

void tune_from_env(Tuning &t) {
    for (const auto &k : TUNE_KEYS)
        if (const char *e = std::getenv(env_name(k.name).c_str()); e && *e) t.*k.mem = std::atoi(e);
    // (a renamed or removed switch must not be silently ignored)
    static bool warned = false;   // once per process, every retired variable that is set
    for (const char *k : RETIRED_KEYS) {
        const std::string var = env_name(k);
        if (!warned && std::getenv(var.c_str()))
            std::fprintf(stderr, "vtkrylov: %s is set but no longer has an effect (retired tuning switch, DESIGN.md §3f)\n",
                         var.c_str());
    }
    warned = true;
}

// host <-> device staging for the *_HOST forms
struct Staged {
    vtk_ctx *c;
    DBuf buf;
    double *d = nullptr;
};

int stage_in(vtk_ctx *c, const double *src, int64_t n, int kind, Staged &s) {
    s.c = c;
    if (kind == VTK_PTR_DEVICE) { s.d = const_cast<double *>(src); return VTK_OK; }
    TRY(dalloc(c, s.buf, std::max<int64_t>(n, 1) * sizeof(double)));
    s.d = s.buf.as<double>();
    if (n && src) HIPCHK(c, hipMemcpyAsync(s.d, src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return VTK_OK;
}

// after the launches of a *_HOST / *_DEVICE entry: the profile folded, a host result copied back
int stage_out(vtk_ctx *c, double *dst, const Staged &s, int64_t n, int kind) {
    if (c->prof_on) prof_flush(c);
    if (kind != VTK_PTR_HOST) return VTK_OK;
    HIPCHK(c, hipMemcpyAsync(dst, s.d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

// the solvers' common entry: argument checks, b and x staged, the solve, x back to the host
template <typename Run>
int staged_solve(const std::string &who, vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
                        int kind, int *info, Run run) {
    if (!A || !b || !x || !info) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    if (M && M->A != A) return fail(c, VTK_ERR_ARG, who + ": preconditioner built for another operator");
    TRY(prec_usable(M, who.c_str()));
    if (!(rtol >= 0.0) || !(atol >= 0.0)) return fail(c, VTK_ERR_ARG, who + ": tolerances must be non-negative");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = A->n_local;
    Staged sb, sx;
    TRY(stage_in(c, b, n, kind, sb));
    TRY(stage_in(c, x, n, kind, sx));
    TRY(run(sb.d, sx.d));
    if (kind == VTK_PTR_HOST) HIPCHK(c, hipMemcpyAsync(x, sx.d, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

// a new preconditioner of A: `fill` allocates and factors it; destroyed again unless every step succeeded
template <typename Fill>
int make_prec(vtk_csr *A, int kind, int bs, vtk_prec **out, Fill fill) {
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    auto *M = new vtk_prec();
    prec_register(M);
    struct Guard { vtk_prec *&m; ~Guard() { if (m) vtk_prec_destroy(m); } } g{M};
    M->A = A;
    M->device = c->device;
    M->kind = kind;
    M->bs = bs;
    TRY(fill(M));
    M->epoch = A->values_epoch;
    *out = M;
    M = nullptr;
    return VTK_OK;
}

// factors copied out to a host or device array, once the stream is idle
int copy_out(vtk_ctx *c, void *dst, const void *src, size_t bytes, int kind) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bytes) HIPCHK(c, hipMemcpy(dst, src, bytes, kind == VTK_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return VTK_OK;
}

}  // namespace

extern "C" {

int vtk_last_error(vtk_ctx *ctx, char *buf, size_t len) {
    if (!buf || len == 0) return VTK_ERR_ARG;
    const std::string e = ctx ? ctx->err : context_free_error();
    std::snprintf(buf, len, "%s", e.c_str());
    return VTK_OK;
}

int vtk_device_count(int *count) {
    if (!count) return VTK_ERR_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *count = n;
    return VTK_OK;
}

int vtk_ctx_create(int device, vtk_ctx **out) {
    if (!out) return fail(nullptr, VTK_ERR_ARG, "vtk_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(nullptr, VTK_ERR_NODEVICE, "vtk_ctx_create: no HIP device visible (the product has no CPU fallback)");
    if (device < 0 || device >= n) return fail(nullptr, VTK_ERR_ARG, "vtk_ctx_create: bad device ordinal");
    auto *c = new vtk_ctx();
    c->device = device;
    tune_from_env(c->tune);   // the only place the library reads its environment
    auto bad = [&](hipError_t e) {
        set_context_free_error(std::string("vtk_ctx_create: ") + hipGetErrorString(e));
        vtk_ctx_destroy(c);
        return e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bad(e);
    if ((e = hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return bad(e);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bad(e);
    if ((e = hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking)) != hipSuccess) return bad(e);
    if ((e = hipEventCreateWithFlags(&c->ev_pack, hipEventDisableTiming)) != hipSuccess) return bad(e);
    if ((e = hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming)) != hipSuccess) return bad(e);
    if ((e = hipMalloc(&c->d_part, 8 * GMAX * sizeof(double))) != hipSuccess) return bad(e);
    if ((e = hipMalloc(&c->d_scal, 256 * sizeof(double))) != hipSuccess) return bad(e);
    if ((e = hipMalloc(&c->d_state, sizeof(GmresState))) != hipSuccess) return bad(e);
    if ((e = hipHostMalloc(&c->h_state, sizeof(GmresState), hipHostMallocDefault)) != hipSuccess) return bad(e);
    if ((e = hipHostMalloc(&c->h_stop, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess) return bad(e);
    if ((e = hipHostGetDevicePointer((void **)&c->d_stop, c->h_stop, 0)) != hipSuccess) return bad(e);
    *c->h_stop = BIG_COL;
    *out = c;
    return VTK_OK;
}

void vtk_ctx_destroy(vtk_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // a communicator whose collective failed may have peers blocked in it: abort, do not destroy
    if (c->comm) (void)(c->comm_broken ? ncclCommAbort(c->comm) : ncclCommDestroy(c->comm));
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    prof_flush(c);
    for (auto e : c->prof_pool) (void)hipEventDestroy(e);
    (void)hipFree(c->d_part);
    (void)hipFree(c->d_scal);
    (void)hipFree(c->d_state);
    if (c->ws) (void)hipFree(c->ws);
    if (c->cap) (void)hipFree(c->cap);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->h_stop) (void)hipHostFree(c->h_stop);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    if (c->ev_pack) (void)hipEventDestroy(c->ev_pack);
    if (c->ev_halo) (void)hipEventDestroy(c->ev_halo);
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int vtk_ctx_stream(vtk_ctx *c, void **stream) {
    if (!c || !stream) return VTK_ERR_ARG;
    *stream = (void *)c->stream;
    return VTK_OK;
}

int vtk_ctx_synchronize(vtk_ctx *c) {
    if (!c) return VTK_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

int vtk_comm_unique_id(void *out128) {
    if (!out128) return fail(nullptr, VTK_ERR_ARG, "vtk_comm_unique_id: NULL");
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(nullptr, VTK_ERR_RCCL, ncclGetErrorString(r));
    std::memcpy(out128, &id, sizeof(id));
    return VTK_OK;
}

int vtk_comm_init(vtk_ctx *c, int rank, int world, const void *uid) {
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(c, VTK_ERR_ARG, "vtk_comm_init: bad rank/world");
    HIPCHK(c, hipSetDevice(c->device));
    // world 1: no communicator, unless tuning comm_solo (VTK_COMM_SOLO=1) asks for a one-rank RCCL communicator
    // that runs every distributed code path (halo plan and exchange, all-reduces, split lists)
    const bool force = world == 1 && c->tune.comm_solo;
    if (world == 1 && !force) { c->rank = 0; c->world = 1; c->dist = false; return VTK_OK; }
    if (!uid) return fail(c, VTK_ERR_ARG, "vtk_comm_init: unique id required");
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    NCCLCHK(c, ncclCommInitRank(&c->comm, world, id, rank));
    c->rank = rank;
    c->world = world;
    c->dist = true;
    return VTK_OK;
}

int vtk_comm_init_host(vtk_ctx *c, int rank, int world, const vtk_host_comm *ops) {
    if (!c || world < 1 || rank < 0 || rank >= world) return fail(c, VTK_ERR_ARG, "vtk_comm_init_host: bad rank/world");
    if (world > 1 && (!ops || !ops->allreduce_sum_f64 || !ops->alltoallv || !ops->allgather))
        return fail(c, VTK_ERR_ARG, "vtk_comm_init_host: all three hooks are required");
    if (c->comm) return fail(c, VTK_ERR_STATE, "vtk_comm_init_host: RCCL communicator already set");
    c->rank = rank;
    c->world = world;
    c->host_comm = world > 1;
    c->dist = world > 1;
    if (ops) c->hops = *ops;
    return VTK_OK;
}

int vtk_comm_info(vtk_ctx *c, int *rank, int *world) {
    if (!c || !rank || !world) return VTK_ERR_ARG;
    *rank = c->rank;
    *world = c->world;
    return VTK_OK;
}

int vtk_comm_rccl_count(vtk_ctx *c, int *count) {
    if (!c || !count) return VTK_ERR_ARG;
    *count = 0;
    if (c->comm) NCCLCHK(c, ncclCommCount(c->comm, count));
    return VTK_OK;
}

int vtk_csr_create(vtk_ctx *c, int64_t n_global, const int64_t *offsets, int64_t nnz,
                   const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                   int kind, vtk_csr **out) {
    if (!c || !out || n_global < 0 || nnz < 0 || !indptr || (nnz > 0 && (!indices || !data)))
        return fail(c, VTK_ERR_ARG, "vtk_csr_create: invalid arguments");
    if (nnz >= ((int64_t)1 << 31)) return fail(c, VTK_ERR_ARG, "vtk_csr_create: nnz must fit int32");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> offs;
    TRY(check_partition(c, n_global, offsets, offs));
    auto *A = new vtk_csr();
    struct Guard { vtk_csr *&a; ~Guard() { if (a) destroy_csr(a); } } g{A};
    A->ctx = c;
    A->device = c->device;
    A->n_global = n_global;
    A->offsets = offs;
    A->row_begin = offs[c->rank];
    A->row_end = offs[c->rank + 1];
    A->n_local = A->row_end - A->row_begin;
    A->nnz = nnz;
    A->fp32 = fp32 ? 1 : 0;
    const int64_t nl = A->n_local;
    A->h_indptr.resize(nl + 1);
    const hipMemcpyKind k = kind == VTK_PTR_DEVICE ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
    HIPCHK(c, hipMemcpy(A->h_indptr.data(), indptr, (nl + 1) * sizeof(int32_t), k));
    if (A->h_indptr[0] != 0 || A->h_indptr[nl] != nnz) return fail(c, VTK_ERR_ARG, "vtk_csr_create: indptr must start at 0 and end at nnz");
    for (int64_t i = 0; i < nl; ++i)
        if (A->h_indptr[i + 1] < A->h_indptr[i]) return fail(c, VTK_ERR_ARG, "vtk_csr_create: indptr not monotone");
    if (kind == VTK_PTR_HOST) {
        for (int64_t kk = 0; kk < nnz; ++kk)
            if (indices[kk] < 0 || indices[kk] >= n_global) return fail(c, VTK_ERR_ARG, "vtk_csr_create: column index out of range");
    }
    const size_t vb = fp32 ? sizeof(float) : sizeof(double);
    HIPCHK(c, hipMalloc(&A->d_indptr, (nl + 1) * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&A->d_indices, std::max<int64_t>(nnz, 1) * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&A->d_data, std::max<int64_t>(nnz, 1) * vb));
    const hipMemcpyKind kd = kind == VTK_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPCHK(c, hipMemcpy(A->d_indptr, A->h_indptr.data(), (nl + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    if (nnz) {
        HIPCHK(c, hipMemcpy(A->d_indices, indices, nnz * sizeof(int32_t), kd));
        HIPCHK(c, hipMemcpy(A->d_data, data, nnz * vb, kd));
        // device-to-device copies on the null stream: complete before the context's
        // (non-blocking) stream reads the arrays
        if (kind == VTK_PTR_DEVICE) HIPCHK(c, hipStreamSynchronize(nullptr));
    }
    if (kind == VTK_PTR_DEVICE && nnz) {   // device input: the same range check on the device
        DBuf mmb;
        TRY(dalloc(c, mmb, 2 * sizeof(int)));
        int mm[2] = {INT_MAX, INT_MIN};
        HIPCHK(c, hipMemcpy(mmb.p, mm, sizeof(mm), hipMemcpyHostToDevice));
        HIPCHK(c, launch_index_range(A->d_indices, nnz, mmb.as<int>(), c->stream));
        TRY(read_back(c, mm, mmb.p));
        if (mm[0] < 0 || (int64_t)mm[1] >= n_global)
            return fail(c, VTK_ERR_ARG, "vtk_csr_create: column index out of range");
    }
    TRY(finish_csr(A));
    // the drop-in path gets the fast solver too: the 2D / 4D Vlasov structure is found in the CSR
    TRY(auto_line_band(A));
    if (A->band_L == 0) TRY(auto_grid4(A));
    *out = A;
    A = nullptr;
    return VTK_OK;
}

int vtk_csr_create_vlasov(vtk_ctx *c, const vtk_vlasov_params *p, const int64_t *offsets, vtk_csr **out) {
    if (!c || !out || !vlasov_params_ok(p)) return fail(c, VTK_ERR_ARG, "vtk_csr_create_vlasov: invalid arguments");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t N = vlasov_n(*p);
    if (vlasov_nnz(*p) >= ((int64_t)1 << 31)) return fail(c, VTK_ERR_ARG, "vtk_csr_create_vlasov: nnz must fit int32");
    std::vector<int64_t> offs;
    TRY(check_partition(c, N, offsets, offs));
    auto *A = new vtk_csr();
    struct Guard { vtk_csr *&a; ~Guard() { if (a) destroy_csr(a); } } g{A};
    A->ctx = c;
    A->device = c->device;
    A->n_global = N;
    A->offsets = offs;
    A->row_begin = offs[c->rank];
    A->row_end = offs[c->rank + 1];
    A->n_local = A->row_end - A->row_begin;
    A->fp32 = p->fp32 ? 1 : 0;
    const int64_t nl = A->n_local;
    HIPCHK(c, hipMalloc(&A->d_indptr, (nl + 1) * sizeof(int32_t)));
    HIPCHK(c, launch_vlasov_counts(*p, A->row_begin, nl, A->d_indptr, c->stream));
    size_t tb = 0;
    HIPCHK(c, launch_exclusive_scan(nullptr, nullptr, nl + 1, nullptr, &tb, c->stream));
    DBuf tmp, cnt;
    TRY(dalloc(c, tmp, tb));
    TRY(dalloc(c, cnt, (nl + 1) * sizeof(int32_t)));
    HIPCHK(c, hipMemcpyAsync(cnt.p, A->d_indptr, (nl + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, launch_exclusive_scan(cnt.as<int32_t>(), A->d_indptr, nl + 1, tmp.p, &tb, c->stream));
    A->h_indptr.resize(nl + 1);
    HIPCHK(c, hipMemcpyAsync(A->h_indptr.data(), A->d_indptr, (nl + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    A->nnz = A->h_indptr[nl];
    const size_t vb = A->fp32 ? sizeof(float) : sizeof(double);
    HIPCHK(c, hipMalloc(&A->d_indices, std::max<int64_t>(A->nnz, 1) * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&A->d_data, std::max<int64_t>(A->nnz, 1) * vb));
    HIPCHK(c, launch_vlasov_fill(*p, A->row_begin, nl, A->d_indptr, A->d_indices, A->d_data, c->stream));
    TRY(finish_csr(A));
    // the 2D operator's rows form x-lines of Nv rows coupled to the neighbouring lines only
    if (p->dim == 2) {
        const int brc = band_check_all(A, p->shape[1]);
        if (brc == VTK_OK) A->band_L = p->shape[1];
        else if (brc != VTK_ERR_ARG) return brc;
    }
    // the 4D operator's rows are grid rows (couplings by one coordinate each)
    if (p->dim == 4) {
        const int grc = grid4_set(A, p->shape[1], p->shape[2], p->shape[3]);
        if (grc != VTK_OK && grc != VTK_ERR_ARG) return grc;
    }
    A->from_vlasov = true;   // vtk_csr_update_vlasov regenerates the values of such an operator
    A->vparams = *p;
    *out = A;
    A = nullptr;
    return VTK_OK;
}

int vtk_csr_info(vtk_csr *A, int64_t *n_global, int64_t *row_begin, int64_t *row_end, int64_t *nnz, int64_t *n_halo) {
    if (!A) return VTK_ERR_ARG;
    if (n_global) *n_global = A->n_global;
    if (row_begin) *row_begin = A->row_begin;
    if (row_end) *row_end = A->row_end;
    if (nnz) *nnz = A->nnz;
    if (n_halo) *n_halo = A->n_halo;
    return VTK_OK;
}

int vtk_csr_download(vtk_csr *A, int32_t *indptr, int32_t *indices, void *data) {
    if (!A || !indptr || (A->nnz && (!indices || !data))) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(indptr, A->h_indptr.data(), A->h_indptr.size() * sizeof(int32_t));
    if (!A->nnz) return VTK_OK;
    HIPCHK(c, hipMemcpy(indices, A->d_indices, A->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(data, A->d_data, A->nnz * (A->fp32 ? sizeof(float) : sizeof(double)), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < A->nnz; ++k) {
        const int64_t l = indices[k];
        indices[k] = (int32_t)(l < A->n_local ? l + A->row_begin : A->halo_cols[l - A->n_local]);
    }
    return VTK_OK;
}

void vtk_csr_destroy(vtk_csr *A) { destroy_csr(A); }

int vtk_csr_update_values(vtk_csr *A, const void *data, int kind) {
    if (!A) return fail(nullptr, VTK_ERR_ARG, "vtk_csr_update_values: A is NULL");
    vtk_ctx *c = A->ctx;
    if ((A->nnz > 0 && !data) || (kind != VTK_PTR_HOST && kind != VTK_PTR_DEVICE))
        return fail(c, VTK_ERR_ARG, "vtk_csr_update_values: invalid arguments");
    HIPCHK(c, hipSetDevice(c->device));
    UpdateScratch u;
    TRY(update_prepare(A, u));
    // first overwrite: the copy runs on the context's stream, behind whatever still reads the old
    // values there (a device array must be complete, as for vtk_csr_create(VTK_PTR_DEVICE))
    if (A->nnz)
        HIPCHK(c, hipMemcpyAsync(A->d_data, data, (size_t)A->nnz * (A->fp32 ? sizeof(float) : sizeof(double)),
                                 kind == VTK_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    return update_finish(A, u);
}

int vtk_csr_update_vlasov(vtk_csr *A, const vtk_vlasov_params *p) {
    if (!A) return fail(nullptr, VTK_ERR_ARG, "vtk_csr_update_vlasov: A is NULL");
    vtk_ctx *c = A->ctx;
    if (!vlasov_params_ok(p)) return fail(c, VTK_ERR_ARG, "vtk_csr_update_vlasov: invalid parameters");
    if (!A->from_vlasov) return fail(c, VTK_ERR_STATE, "vtk_csr_update_vlasov: the operator was not made by vtk_csr_create_vlasov");
    const vtk_vlasov_params &q = A->vparams;
    bool same = p->dim == q.dim && (p->fp32 != 0) == (q.fp32 != 0);
    for (int k = 0; k < (p->dim == 4 ? 4 : p->dim) && same; ++k) same = p->shape[k] == q.shape[k];
    if (!same) return fail(c, VTK_ERR_ARG, "vtk_csr_update_vlasov: dim, shape and fp32 must equal the creating parameters");
    HIPCHK(c, hipSetDevice(c->device));
    UpdateScratch u;
    TRY(update_prepare(A, u));
    { Prof pf(c, "vlasov_values", -1, 4.0 * (A->n_local + 1) + (A->fp32 ? 4.0 : 8.0) * (double)A->nnz);   // indptr read, values written
      HIPCHK(c, launch_vlasov_values(*p, A->row_begin, A->n_local, A->d_indptr, A->d_data, c->stream)); }
    TRY(update_finish(A, u));
    A->vparams = *p;
    return VTK_OK;
}

int vtk_csr_values_epoch(vtk_csr *A, int64_t *epoch) {
    if (!A || !epoch) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_csr_values_epoch: NULL argument");
    *epoch = A->values_epoch;
    return VTK_OK;
}

int vtk_spmv(vtk_csr *A, const double *x, double *y, int kind) {
    if (!A || !x || !y) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    Staged sx, sy;
    TRY(stage_in(c, x, A->n_local, kind, sx));
    TRY(stage_in(c, kind == VTK_PTR_DEVICE ? y : nullptr, A->n_local, kind, sy));
    TRY(halo_exchange(A, sx.d));
    { Prof pf(c, "spmv", -1, matrix_bytes(A) + 16.0 * A->n_local);
      HIPCHK(c, launch_spmv(spmv_in(A, &A->tiles, sx.d), EPI_PLAIN, sy.d, nullptr, BjOp{}, nullptr, nullptr, nullptr, nullptr, 0, c->stream)); }
    return stage_out(c, y, sy, A->n_local, kind);
}

int vtk_bjacobi_create(vtk_csr *A, int bs, vtk_prec **out) { return vtk_bjacobi_create_ex(A, bs, VTK_BJ_SETUP_EXACT, out); }

int vtk_bjacobi_create_ex(vtk_csr *A, int bs, int setup, vtk_prec **out) {
    if (!A || !out || bs < 1 || bs > 64) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_bjacobi_create: block size must be in [1, 64]");
    if (setup != VTK_BJ_SETUP_EXACT && setup != VTK_BJ_SETUP_MFMA && setup != VTK_BJ_SETUP_AUTO)
        return fail(A->ctx, VTK_ERR_ARG, "vtk_bjacobi_create_ex: unknown setup");
    if (setup == VTK_BJ_SETUP_AUTO) setup = (bs == 16 || bs == 32) ? VTK_BJ_SETUP_MFMA : VTK_BJ_SETUP_EXACT;
    if (setup == VTK_BJ_SETUP_MFMA && bs != 16 && bs != 32)
        return fail(A->ctx, VTK_ERR_ARG, "vtk_bjacobi_create_ex: the MFMA setup takes bs 16 or 32");
    vtk_ctx *c = A->ctx;
    *out = nullptr;
    if (A->row_begin % bs != 0) return fail(c, VTK_ERR_ARG, "vtk_bjacobi_create: rank row block must start at a multiple of the block size");
    return make_prec(A, VTK_PREC_BJACOBI, bs, out, [&](vtk_prec *M) -> int {
        M->nb = (A->n_local + bs - 1) / bs;
        M->setup = setup;
        HIPCHK(c, hipMalloc(&M->d_inv, std::max<int64_t>(M->nb, 1) * bs * bs * sizeof(double)));
        TRY(bj_factor(M));
        if ((bs & (bs - 1)) != 0 || bs > 32) return VTK_OK;
        std::vector<int32_t> rows;
        TRY(upload_tiles(c, A->h_indptr, bs, M->tiles, &rows));
        M->fused = M->tiles.aligned && !M->tiles.has_long;
        if (M->fused && c->dist && A->row_halo.size() == (size_t)A->n_local) {
            TRY(upload_split_tiles(c, rows, A->row_halo, M->tiles, M->tiles_in, M->tiles_bd));
            M->split = true;
        }
        return VTK_OK;
    });
}

int vtk_linejacobi_create(vtk_csr *A, int64_t stride, int64_t seg, vtk_prec **out) {
    if (!A || !out) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    *out = nullptr;
    if (stride < 1 || seg < 1) return fail(c, VTK_ERR_ARG, "vtk_linejacobi_create: stride and seg must be >= 1");
    if (A->n_global > 0 && stride >= A->n_global && A->n_global > 1)
        return fail(c, VTK_ERR_ARG, "vtk_linejacobi_create: stride must be below n (no line has two rows)");
    return make_prec(A, VTK_PREC_LINE, 0, out, [&](vtk_prec *M) -> int {
        M->line = line_plan(A->n_local, A->row_begin, stride, seg);
        HIPCHK(c, hipMalloc(&M->line.f, 3 * std::max<int64_t>(A->n_local, 1) * sizeof(double)));
        return line_factor(M);
    });
}

int vtk_lineproduct_create(vtk_csr *A, int64_t stride1, int64_t seg1, int64_t stride2, int64_t seg2, vtk_prec **out) {
    if (!A || !out) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    *out = nullptr;
    if (stride1 < 1 || seg1 < 1 || stride2 < 1 || seg2 < 1)
        return fail(c, VTK_ERR_ARG, "vtk_lineproduct_create: strides and segs must be >= 1");
    if (A->n_global > 1 && (stride1 >= A->n_global || stride2 >= A->n_global))
        return fail(c, VTK_ERR_ARG, "vtk_lineproduct_create: the strides must be below n (no line has two rows)");
    return make_prec(A, VTK_PREC_LINE2, 0, out, [&](vtk_prec *M) -> int {
        const int64_t n1 = std::max<int64_t>(A->n_local, 1);
        M->line = line_plan(A->n_local, A->row_begin, stride1, seg1);
        M->line2 = line_plan(A->n_local, A->row_begin, stride2, seg2);
        HIPCHK(c, hipMalloc(&M->line.f, 3 * n1 * sizeof(double)));
        HIPCHK(c, hipMalloc(&M->line2.f, 3 * n1 * sizeof(double)));
        HIPCHK(c, hipMalloc(&M->d_diag, n1 * sizeof(double)));
        return line2_factor(M);
    });
}

int vtk_linecyclic_create(vtk_csr *A, int64_t stride, int64_t period, int64_t seg, vtk_prec **out) {
    if (!A || !out) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    *out = nullptr;
    if (stride < 1 || period < 3 || seg < 2)
        return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create: stride must be >= 1, period >= 3 and seg >= 2");
    if (stride > INT64_MAX / period || A->row_begin % (stride * period) != 0 || A->n_local % (stride * period) != 0)
        return fail(c, VTK_ERR_ARG, "vtk_linecyclic_create: the rank's first row and row count must be multiples of stride * "
                                    "period (every cyclic line on one rank)");
    return make_prec(A, VTK_PREC_LINEC, 0, out, [&](vtk_prec *M) -> int {
        TRY(linec_plan(M, stride, period, seg));
        return linec_factor(M);
    });
}

int vtk_linecyclic_create_span(vtk_csr *A, int64_t stride, int64_t period, int64_t seg, vtk_prec **out) {
    if (!A || !out) return VTK_ERR_ARG;
    *out = nullptr;
    // collective: the arguments are judged inside, from what every rank contributes
    return make_prec(A, VTK_PREC_LINEC, 0, out, [&](vtk_prec *M) -> int {
        TRY(linec_span_plan(M, stride, period, seg));
        return linec_factor(M);
    });
}

int vtk_linecyclic_span_info(vtk_prec *M, vtk_linec_span_info *out) {
    if (!M || !out) return VTK_ERR_ARG;
    if (M->kind != VTK_PREC_LINEC || !M->linec.sp.on)
        return fail(M->A->ctx, VTK_ERR_STATE, "vtk_linecyclic_span_info: not a cyclic-line preconditioner that spans the ranks");
    const LineCSpan &sp = M->linec.sp;
    vtk_linec_span_info o{};
    o.world = sp.world;
    o.rank = sp.rank;
    o.spanning = 1;
    o.first_line = sp.i0;
    o.local_period = M->linec.period;
    o.period = sp.gperiod;
    *out = o;
    return VTK_OK;
}

int vtk_linecyclic_info(vtk_prec *M, vtk_linec_info *out) {
    if (!M || !out) return VTK_ERR_ARG;
    if (M->kind != VTK_PREC_LINEC) return fail(M->A->ctx, VTK_ERR_STATE, "vtk_linecyclic_info: not a cyclic-line preconditioner");
    const LineC &C = M->linec;
    vtk_linec_info o{};
    o.levels = C.nlev;
    o.compact = 0;   // the spikes are stored per row
    o.stride = C.stride;
    o.period = C.sp.on ? C.sp.gperiod : C.period;   // (spanning: unknowns[0] is the rank's share of it)
    o.seg = C.seg;
    for (int k = 0; k < C.nlev && k < 32; ++k) o.unknowns[k] = C.lev[k].period;
    *out = o;
    return VTK_OK;
}

int vtk_lineproduct_factors(vtk_prec *M, int which, double *f, int kind) {
    if (!M || !f) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    if (M->kind != VTK_PREC_LINE2) return fail(c, VTK_ERR_STATE, "vtk_lineproduct_factors: not a line-product preconditioner");
    if (which < 0 || which > 2) return fail(c, VTK_ERR_ARG, "vtk_lineproduct_factors: which must be 0, 1 (l|m|g of a direction) or 2 (D)");
    TRY(prec_usable(M, "vtk_lineproduct_factors"));
    const double *src = which == 0 ? M->line.f : which == 1 ? M->line2.f : M->d_diag;
    return copy_out(c, f, src, (which == 2 ? 1 : 3) * M->A->n_local * sizeof(double), kind);
}

int vtk_linejacobi_factors(vtk_prec *M, double *f, int kind) {
    if (!M || !f) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    if (M->kind != VTK_PREC_LINE) return fail(c, VTK_ERR_STATE, "vtk_linejacobi_factors: not a line-Jacobi preconditioner");
    TRY(prec_usable(M, "vtk_linejacobi_factors"));
    return copy_out(c, f, M->line.f, 3 * M->line.n * sizeof(double), kind);
}

int vtk_linejacobi_set_compact(vtk_prec *M, int on) {
    if (!M) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    if (M->kind != VTK_PREC_LINE) return fail(c, VTK_ERR_STATE, "vtk_linejacobi_set_compact: not a line-Jacobi preconditioner");
    if (on && !M->line_compact_ok) return fail(c, VTK_ERR_ARG, "vtk_linejacobi_set_compact: the x-couplings are not constant along the lines");
    M->line.compact = on ? 1 : 0;
    M->compact_req = on ? 1 : 0;   // vtk_prec_refresh keeps a set_compact(0)
    return VTK_OK;
}

int vtk_linejacobi_get_compact(vtk_prec *M, int *in_use, int *available) {
    if (!M) return VTK_ERR_ARG;
    if (M->kind != VTK_PREC_LINE) return fail(M->A->ctx, VTK_ERR_STATE, "vtk_linejacobi_get_compact: not a line-Jacobi preconditioner");
    if (in_use) *in_use = M->line.compact;
    if (available) *available = M->line_compact_ok ? 1 : 0;
    return VTK_OK;
}

int vtk_prec_apply(vtk_prec *M, const double *r, double *z, int kind) { return vtk_bjacobi_apply(M, r, z, kind); }

int vtk_neumann_create(vtk_csr *A, vtk_prec *base, int degree, vtk_prec **out) {
    vtk_ctx *c = A ? A->ctx : nullptr;
    if (degree < 1 || degree > 8) return fail(c, VTK_ERR_ARG, "vtk_neumann_create: degree must be in [1, 8]");
    if (!A || !base || !out) return fail(c, VTK_ERR_ARG, "vtk_neumann_create: NULL argument");
    *out = nullptr;
    if (!prec_alive(base, 0)) return fail(c, VTK_ERR_STATE, "vtk_neumann_create: the base preconditioner has been destroyed");
    if (base->kind == VTK_PREC_NEUMANN) return fail(c, VTK_ERR_ARG, "vtk_neumann_create: the base is itself a Neumann wrapper (no nesting)");
    if (base->A != A) return fail(c, VTK_ERR_ARG, "vtk_neumann_create: the base preconditioner was built for another operator");
    if (base->kind == VTK_PREC_LINEC && base->linec.sp.on)
        return fail(c, VTK_ERR_ARG, "vtk_neumann_create: cyclic lines that span the ranks are not taken as a base");
    TRY(prec_usable(base, "vtk_neumann_create"));
    const int rc = make_prec(A, VTK_PREC_NEUMANN, 0, out, [&](vtk_prec *M) -> int {
        M->base = base;
        M->base_id = base->id;
        M->degree = degree;
        // z_i alternate between two vectors, t = r - A z_i in the third (64-row padding: 16-byte rows)
        const int64_t ld = round_up(std::max<int64_t>(A->n_local, 1), 64);
        if (degree > 1) HIPCHK(c, hipMalloc(&M->d_neu, 3 * (size_t)ld * sizeof(double)));
        return VTK_OK;
    });
    if (rc == VTK_OK) (*out)->epoch = base->epoch;   // the wrapper's epoch is its base's
    return rc;
}

int vtk_neumann_info(vtk_prec *M, vtk_neu_info *out) {
    if (!M || !out) return VTK_ERR_ARG;
    if (M->kind != VTK_PREC_NEUMANN) return fail(M->A->ctx, VTK_ERR_STATE, "vtk_neumann_info: not a Neumann wrapper");
    vtk_neu_info o{};
    o.degree = M->degree;
    o.base_alive = prec_alive(M->base, M->base_id) ? 1 : 0;
    o.base_kind = o.base_alive ? M->base->kind : -1;
    o.fused = o.base_alive && M->degree > 1 && neu_fused(M) ? 1 : 0;
    *out = o;
    return VTK_OK;
}

// w = M^-1 A x through the launch the solver's split DCGS2 step uses for this operator (ADVICE r5:
// the kernel-level pin of k_g4_ring against k_sell<EPI_PREC>): the 4D ring kernel when it applies
// -- across ranks in the solver's form, interior groups while the halo planes travel, then the
// first / last planes' groups --, else the SELL / CSR SpMV with the BJ epilogue, else SpMV + apply
int vtk_precond_matvec(vtk_csr *A, vtk_prec *M, const double *x, double *w, int kind) {
    if (!A || !x || !w || (M && M->A != A)) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_precond_matvec: bad arguments");
    vtk_ctx *c = A->ctx;
    TRY(prec_usable(M, "vtk_precond_matvec"));
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = A->n_local;
    Staged sx, sw;
    TRY(stage_in(c, x, n, kind, sx));
    TRY(stage_in(c, kind == VTK_PTR_DEVICE ? w : nullptr, n, kind, sw));
    const bool ring = g4_ring_ok(c, A, M);
    double *p0 = c->d_part, *p1 = c->d_part + GMAX;
    if (ring) {
        const double *halo = A->g4.lblk >= 0 ? A->d_halo : nullptr;
        Prof pf(c, "spmv_bj", -1, solver_matrix_bytes(A) + prec_row_bytes(M) * n + 16.0 * n);
        if (!halo) {
            TRY(halo_exchange(A, sx.d));
            HIPCHK(c, launch_g4_ring(A->g4, sx.d, nullptr, M->d_tri + M->tri_ld, sw.d, n, A->fp32, c->tune.g4_ring,
                                     c->tune.g4_gr, nullptr, nullptr, nullptr, 0, c->stream, 0, -1, 0, c->tune.g4_fast));
        } else {   // the solver's split form without dots: always exchanges, no vote (fails at once), this one bracket
            TRY(g4_ring_split(A, M, sx.d, sw.d, true, nullptr, nullptr, 0.0, nullptr, nullptr, 0, nullptr));
        }
    } else if (line_fuse_ok(c, A, M)) {
        // the line step's form: y = A x formed inside the sweep kernel (k_line_spmv_dc; its step-0
        // dots go to a scratch), the ADVICE r5 pin of the fused kernel against SpMV + sweeps below
        DBuf part;
        TRY(dalloc(c, part, (size_t)DC_NQ * GMAX * sizeof(double)));
        Prof pf(c, "line_dc", -1, prec_row_bytes(M) * n + 24.0 * n);
        HIPCHK(c, launch_line_spmv_dc(M->line, A->d_lsv, sx.d, sw.d, sx.d, n, 0, part.as<double>(), vector_grid(n),
                                      nullptr, 0, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // part is freed on return
    } else if (!M || bj_fused(M)) {
        TRY(halo_exchange(A, sx.d));
        Prof pf(c, M ? "spmv_bj" : "spmv_w", -1, solver_matrix_bytes(A) + prec_row_bytes(M) * n + 16.0 * n);
        HIPCHK(c, launch_spmv(lsv_in(spmv_in(A, M ? &M->tiles : &A->tiles, sx.d), A), EPI_PREC, sw.d, nullptr,
                              M ? bj_op(M) : BjOp{}, nullptr, p0, p1, nullptr, 0, c->stream));
    } else {
        TRY(halo_exchange(A, sx.d));
        DBuf t;
        TRY(dalloc(c, t, std::max<int64_t>(n, 1) * sizeof(double)));
        HIPCHK(c, launch_spmv(lsv_in(spmv_in(A, &A->tiles, sx.d), A), EPI_PLAIN, t.as<double>(), nullptr, BjOp{}, nullptr,
                              nullptr, nullptr, nullptr, 0, c->stream));
        TRY(prec_apply(c, M, n, t.as<double>(), sw.d, nullptr, nullptr, nullptr, vector_grid(n), nullptr, 0, nullptr));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // t is freed on return
    }
    return stage_out(c, w, sw, n, kind);
}

int vtk_prec_refresh(vtk_prec *M, int64_t *epoch) {
    if (!M) return fail(nullptr, VTK_ERR_ARG, "vtk_prec_refresh: M is NULL");
    vtk_csr *A = M->A;
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (M->kind == VTK_PREC_NEUMANN) {   // the wrapper owns no factors: its base's refresh, its base's epoch
        if (!prec_alive(M->base, M->base_id))
            return fail(c, VTK_ERR_STATE, "vtk_prec_refresh: the Neumann wrapper's base preconditioner has been destroyed");
        int64_t eb = M->base->epoch;
        const int rc = vtk_prec_refresh(M->base, &eb);
        M->epoch = M->base->epoch;
        M->valid = M->base->valid;
        if (epoch) *epoch = M->epoch;
        return rc;
    }
    // the factors are overwritten from the first launch on: M is invalid until they are whole again
    const int64_t e = A->values_epoch;
    const int rc = M->kind == VTK_PREC_LINEC ? linec_factor(M) : M->kind == VTK_PREC_LINE2 ? line2_factor(M) : M->kind == VTK_PREC_LINE ? line_factor(M) : bj_factor(M);
    if (rc == VTK_ERR_SINGULAR) M->valid = false;
    if (rc != VTK_OK) return rc;
    M->valid = true;
    M->epoch = e;
    if (epoch) *epoch = e;
    if (M->kind == VTK_PREC_BJACOBI && M->mode == VTK_BJ_TRIDIAG && !M->tri_ok)
        return fail(c, VTK_ERR_ARG, "vtk_prec_refresh: the blocks are no longer tridiagonal (or their factors failed the "
                                    "check): the TRIDIAG request cannot be met, M applies the inverses");
    if (M->kind == VTK_PREC_LINE && M->compact_req == 1 && !M->line_compact_ok)
        return fail(c, VTK_ERR_ARG, "vtk_prec_refresh: the x-couplings are no longer constant along the lines: the "
                                    "COMPACT request cannot be met, M applies the stored factors");
    return VTK_OK;
}

int vtk_prec_kind_of(vtk_prec *M, int *kind) {
    if (!M || !kind) return VTK_ERR_ARG;
    *kind = M->kind;
    return VTK_OK;
}

int vtk_bjacobi_inverse(vtk_prec *M, double *inv, int kind) {
    if (!M || !inv) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    if (M->kind != VTK_PREC_BJACOBI) return fail(c, VTK_ERR_STATE, "vtk_bjacobi_inverse: not a block-Jacobi preconditioner");
    TRY(prec_usable(M, "vtk_bjacobi_inverse"));
    return copy_out(c, inv, M->d_inv, M->nb * M->bs * M->bs * sizeof(double), kind);
}

int vtk_bjacobi_apply(vtk_prec *M, const double *r, double *z, int kind) {
    if (!M || !r || !z) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    TRY(prec_usable(M, "vtk_prec_apply"));
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t n = M->A->n_local;
    Staged sr, sz;
    TRY(stage_in(c, r, n, kind, sr));
    TRY(stage_in(c, kind == VTK_PTR_DEVICE ? z : nullptr, n, kind, sz));
    if (M->kind == VTK_PREC_NEUMANN && kind == VTK_PTR_DEVICE && r == z)
        return fail(c, VTK_ERR_ARG, "vtk_prec_apply: a Neumann wrapper cannot apply in place (r and z alias)");
    { Prof pf(c, prec_cls(M), -1, prec_row_bytes(M) * n + 16.0 * n);
      TRY(prec_apply(c, M, n, sr.d, sz.d, nullptr, nullptr, nullptr, vector_grid(n), nullptr, 0, nullptr)); }
    return stage_out(c, z, sz, n, kind);
}

int vtk_csr_set_layout(vtk_csr *A, int layout) {
    if (!A) return VTK_ERR_ARG;
    vtk_ctx *c = A->ctx;
    if (layout != VTK_LAYOUT_AUTO && layout != VTK_LAYOUT_CSR && layout != VTK_LAYOUT_SELL &&
        layout != VTK_LAYOUT_SELL32)
        return fail(c, VTK_ERR_ARG, "vtk_csr_set_layout: unknown layout");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return apply_layout(A, layout);
}

int vtk_csr_get_layout(vtk_csr *A, int *layout_in_use) {
    if (!A || !layout_in_use) return VTK_ERR_ARG;
    *layout_in_use = A->use_sell ? (A->sell.d_pk ? VTK_LAYOUT_SELL : VTK_LAYOUT_SELL32) : VTK_LAYOUT_CSR;
    return VTK_OK;
}

int vtk_csr_layout_info(vtk_csr *A, vtk_layout_info *out) {
    if (!A || !out) return VTK_ERR_ARG;
    vtk_layout_info li{};
    int lay = VTK_LAYOUT_CSR;
    (void)vtk_csr_get_layout(A, &lay);
    li.layout = lay;
    li.matrix_bytes = matrix_bytes(A);
    li.sell_chunks = A->use_sell ? A->sell.nch : 0;
    li.sell_entries = A->use_sell ? A->sell.entries : 0;
    li.wide_chunks = A->use_sell && A->sell.d_pk ? A->sell.n_wide : 0;
    *out = li;
    return VTK_OK;
}

int vtk_bjacobi_set_mode(vtk_prec *M, int mode) {
    if (!M) return VTK_ERR_ARG;
    vtk_ctx *c = M->A->ctx;
    if (M->kind != VTK_PREC_BJACOBI) return fail(c, VTK_ERR_STATE, "vtk_bjacobi_set_mode: not a block-Jacobi preconditioner");
    if (mode != VTK_BJ_AUTO && mode != VTK_BJ_INVERSE && mode != VTK_BJ_TRIDIAG)
        return fail(c, VTK_ERR_ARG, "vtk_bjacobi_set_mode: unknown mode");
    if (mode == VTK_BJ_TRIDIAG && !M->tri_ok)
        return fail(c, VTK_ERR_ARG, "vtk_bjacobi_set_mode: blocks are not tridiagonal (bs 2/4/8) or their factors failed the check");
    M->mode = mode;
    return VTK_OK;
}

int vtk_bjacobi_get_mode(vtk_prec *M, int *mode_in_use, int *tridiag_available) {
    if (!M) return VTK_ERR_ARG;
    if (M->kind != VTK_PREC_BJACOBI) return fail(M->A->ctx, VTK_ERR_STATE, "vtk_bjacobi_get_mode: not a block-Jacobi preconditioner");
    if (mode_in_use) *mode_in_use = bj_op(M).tri ? VTK_BJ_TRIDIAG : VTK_BJ_INVERSE;
    if (tridiag_available) *tridiag_available = M->tri_ok ? 1 : 0;
    return VTK_OK;
}

void vtk_prec_destroy(vtk_prec *M) {
    if (!M) return;
    prec_unregister(M);   // (a Neumann wrapper that borrowed M finds it gone; its own base is left alone)
    (void)hipSetDevice(M->device);
    (void)hipFree(M->d_neu);
    (void)hipFree(M->d_inv);
    (void)hipFree(M->d_tri);
    (void)hipFree(M->line.f);
    (void)hipFree(M->line.ac);
    (void)hipFree(M->line2.f);
    (void)hipFree(M->line2.ac);
    (void)hipFree(M->d_diag);
    linec_free(M->linec);
    free_tiles(M->tiles);
    free_tiles(M->tiles_in);
    free_tiles(M->tiles_bd);
    delete M;
}

int vtk_csr_set_line_band(vtk_csr *A, int64_t line_len) {
    if (!A) return fail(nullptr, VTK_ERR_ARG, "vtk_csr_set_line_band: A is NULL");
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (line_len == 0) {
        A->band_L = 0;
        return VTK_OK;
    }
    const int rc = band_check_all(A, line_len);
    if (rc == VTK_ERR_ARG)
        return fail(c, VTK_ERR_ARG, "vtk_csr_set_line_band: not a line-band operator for this line length "
                                    "(line_len | n, >= 3 lines, every column in lines x-1..x+1, n + 2 line_len "
                                    "< 2^30; across ranks: slabs of whole lines whose halo is the two neighbour lines)");
    TRY(rc);
    A->band_L = line_len;
    return VTK_OK;
}

int vtk_csr_get_line_band(vtk_csr *A, int64_t *line_len) {
    if (!A || !line_len) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_csr_get_line_band: NULL argument");
    *line_len = A->band_L;
    return VTK_OK;
}

int vtk_csr_set_grid4(vtk_csr *A, int64_t Ny, int64_t Nvx, int64_t Nvy) {
    if (!A) return fail(nullptr, VTK_ERR_ARG, "vtk_csr_set_grid4: A is NULL");
    vtk_ctx *c = A->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if (Ny == 0) {   // clear
        set_grid4_tables(A, Grid4{}, nullptr, nullptr);
        A->g4_try = Grid4{};
        return VTK_OK;
    }
    const int rc = grid4_set(A, Ny, Nvx, Nvy);
    if (rc == VTK_ERR_ARG)
        return fail(c, VTK_ERR_ARG, "vtk_csr_set_grid4: not a 4D grid operator of these extents (rows = whole x planes "
                                    "of Ny*Nvx*Nvy rows, Ny >= 3, Nvx, Nvy >= 2, each row coupled to x+-1, y+-1, "
                                    "vx+-1, vy+-1 in ascending column order with values by one coordinate each)");
    return rc;
}

int vtk_csr_get_grid4(vtk_csr *A, int64_t *dims) {
    if (!A || !dims) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_csr_get_grid4: NULL argument");
    dims[0] = A->d_g4tab ? A->g4.Ny : 0;
    dims[1] = A->d_g4tab ? A->g4.Nvx : 0;
    dims[2] = A->d_g4tab ? A->g4.Nvy : 0;
    return VTK_OK;
}

int vtk_csr_get_line_values(vtk_csr *A, int *separable) {
    if (!A || !separable) return fail(A ? A->ctx : nullptr, VTK_ERR_ARG, "vtk_csr_get_line_values: NULL argument");
    *separable = A->band_L > 0 && A->d_lsv != nullptr ? (A->lsv_canon ? 2 : 1) : 0;
    return VTK_OK;
}

int vtk_gmres_set_band(vtk_ctx *c, int on) {
    if (!c) return fail(nullptr, VTK_ERR_ARG, "vtk_gmres_set_band: ctx is NULL");
    c->tune.band = on != 0;
    return VTK_OK;
}

int vtk_ctx_set_tuning(vtk_ctx *c, const char *key, int value) {
    if (!c) return fail(nullptr, VTK_ERR_ARG, "vtk_ctx_set_tuning: ctx is NULL");
    const TuneKey *k = tune_key(key);
    if (!k) return fail(c, VTK_ERR_ARG, std::string("vtk_ctx_set_tuning: unknown key ") + (key ? key : "(null)"));
    c->tune.*k->mem = value;
    return VTK_OK;
}

int vtk_ctx_get_tuning(vtk_ctx *c, const char *key, int *value) {
    if (!c || !value) return fail(c, VTK_ERR_ARG, "vtk_ctx_get_tuning: NULL argument");
    const TuneKey *k = tune_key(key);
    if (!k) return fail(c, VTK_ERR_ARG, std::string("vtk_ctx_get_tuning: unknown key ") + (key ? key : "(null)"));
    *value = c->tune.*k->mem;
    return VTK_OK;
}

int vtk_gmres_set_orth(vtk_ctx *c, int orth) {
    if (!c || (orth != VTK_ORTH_MGS && orth != VTK_ORTH_DCGS2 && orth != VTK_ORTH_AUTO))
        return fail(c, VTK_ERR_ARG, "vtk_gmres_set_orth: unknown scheme");
    c->orth = orth;
    return VTK_OK;
}

int vtk_gmres_set_basis(vtk_ctx *c, int basis) {
    if (!c || (basis != VTK_BASIS_F64 && basis != VTK_BASIS_F32))
        return fail(c, VTK_ERR_ARG, "vtk_gmres_set_basis: unknown basis storage (VTK_BASIS_F64 or VTK_BASIS_F32)");
    c->basis = basis;
    return VTK_OK;
}

int vtk_gmres_basis_info(vtk_ctx *c, vtk_basis_info *out) {
    if (!c || !out) return fail(c, VTK_ERR_ARG, "vtk_gmres_basis_info: NULL argument");
    *out = c->basis_info;
    out->requested = c->basis;
    return VTK_OK;
}

int vtk_gmres_capture(vtk_ctx *c, int cycle) {
    if (!c || cycle < -2) return fail(c, VTK_ERR_ARG, "vtk_gmres_capture: cycle must be >= 0, -1 (off) or -2 (every cycle)");
    c->cap_cycle = cycle;
    return VTK_OK;
}

int vtk_gmres_captured(vtk_ctx *c, vtk_arnoldi_info *info) {
    if (!c || !info) return VTK_ERR_ARG;
    if (!c->cap_valid) return fail(c, VTK_ERR_STATE, "vtk_gmres_captured: no restart cycle has been captured");
    *info = c->cap_info;
    return VTK_OK;
}

int vtk_gmres_captured_read(vtk_ctx *c, int what, void *dst, int kind) {
    if (!c || !dst || (kind != VTK_PTR_HOST && kind != VTK_PTR_DEVICE)) return fail(c, VTK_ERR_ARG, "vtk_gmres_captured_read: bad argument");
    if (!c->cap_valid) return fail(c, VTK_ERR_STATE, "vtk_gmres_captured_read: no restart cycle has been captured");
    const vtk_arnoldi_info &ci = c->cap_info;
    const size_t m = (size_t)ci.restart, ld = (size_t)ci.ld;
    const double *V = c->cap + ld, *H = V + (m + 1) * ld, *S = H + m * (m + 1), *giv = S + (m + 1);
    const double *Hraw = giv + 2 * m;
    const DcCoef *cf = reinterpret_cast<const DcCoef *>(Hraw + (m + 1) * (m + 1));
    const void *src = nullptr;
    size_t bytes = 0;
    switch (what) {
    case VTK_CAP_V: src = V; bytes = (m + 1) * ld * sizeof(double); break;
    case VTK_CAP_X_IN: src = c->cap; bytes = (size_t)ci.n_local * sizeof(double); break;
    case VTK_CAP_H: src = H; bytes = m * (m + 1) * sizeof(double); break;
    case VTK_CAP_S: src = S; bytes = (m + 1) * sizeof(double); break;
    case VTK_CAP_GIV: src = giv; bytes = 2 * m * sizeof(double); break;
    case VTK_CAP_HRAW: src = Hraw; bytes = (m + 1) * (m + 1) * sizeof(double); break;
    case VTK_CAP_COMMITTED: src = cf->committed; bytes = (m + 1) * sizeof(int); break;
    case VTK_CAP_NU: src = &cf->nu; bytes = sizeof(double); break;
    default: return fail(c, VTK_ERR_ARG, "vtk_gmres_captured_read: unknown item");
    }
    if (what >= VTK_CAP_HRAW && !ci.has_hraw) return fail(c, VTK_ERR_STATE, "vtk_gmres_captured_read: the captured cycle ran MGS (no Hraw)");
    if (bytes == 0) return VTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind == VTK_PTR_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

int vtk_profile_enable(vtk_ctx *c, int on) {
    if (!c) return VTK_ERR_ARG;
    prof_flush(c);
    c->prof_on = on != 0;
    if (c->prof_on) c->prof_acc.clear();
    return VTK_OK;
}

int vtk_profile_read(vtk_ctx *c, vtk_kernel_profile *out, int max_entries, int *n_entries) {
    if (!c || !n_entries || (max_entries > 0 && !out)) return VTK_ERR_ARG;
    prof_flush(c);
    *n_entries = (int)c->prof_acc.size();
    for (int i = 0; i < max_entries && i < (int)c->prof_acc.size(); ++i) {
        const auto &a = c->prof_acc[i];
        std::snprintf(out[i].name, sizeof(out[i].name), "%s", a.name.c_str());
        out[i].launches = a.launches;
        out[i].seconds = a.seconds;
        out[i].bytes = a.bytes;
    }
    return VTK_OK;
}

int vtk_gmres(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
              int restart, int64_t maxiter, int kind, int *info, vtk_stats *st) {
    return staged_solve("vtk_gmres", A, M, b, x, rtol, atol, kind, info, [&](const double *db, double *dx) {
        return run_gmres(A, M, db, dx, rtol, atol, restart, maxiter, info, st); });
}

int vtk_bicgstab(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol, int64_t maxiter,
                 int kind, int *info, vtk_bicgstab_stats *st) {
    return staged_solve("vtk_bicgstab", A, M, b, x, rtol, atol, kind, info, [&](const double *db, double *dx) {
        return run_bicgstab(A, M, db, dx, rtol, atol, maxiter, info, st); });
}

}  // extern "C"
