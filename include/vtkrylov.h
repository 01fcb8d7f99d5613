/* vtkrylov.h — C-ABI of libvtkrylov.so, the MI355X-native preconditioned-Krylov path.
 *
 * Boundary.  jwang1x/VT-precondition has no solver, no FFI and no plugin
 * interface (the reference is Python provisioning scripts only).  The
 * entry points below replace the calls the north_star's "reference scipy.sparse path"
 * makes — the reference-side binding a maintainer adds is the ctypes stub in
 * INTEGRATION.md (vtkrylov/_abi.py in this repo) — and each declaration names the SciPy
 * interface it stands in for:
 *   vtk_csr_create      <- scipy.sparse.csr_matrix((data, indices, indptr), shape)
 *                          (scipy/sparse/_compressed.py _cs_matrix.__init__)
 *   vtk_spmv            <- csr_matrix @ x -> _matmul_vector (scipy/sparse/_compressed.py:518-530)
 *   vtk_bjacobi_create  <- numpy.linalg.inv on the bs x bs diagonal blocks
 *   vtk_bjacobi_apply   <- LinearOperator(matvec=einsum('bij,bj->bi'))
 *   vtk_linejacobi_*    <- LinearOperator(matvec=splu(M).solve), M = diagonal + x-line
 *                          couplings (line-implicit x-direction solve)
 *   vtk_lineproduct_*   <- LinearOperator(matvec=lambda r: lu2.solve(D * lu1.solve(r))),
 *                          lu_i = splu(M_i): two line directions
 *   vtk_linecyclic_*    <- LinearOperator(matvec=splu(M).solve), M = diagonal + the periodic
 *                          lines' couplings, wrap included
 *   vtk_neumann_*       <- LinearOperator(matvec=mv), mv(r): z = M(r); degree - 1 times
 *                          z = z + M(r - A @ z) -- the Neumann series of M^-1 A around any of the
 *                          preconditioners above
 *   vtk_gmres          <- scipy.sparse.linalg.gmres(A, b, x0, rtol=, atol=, restart=,
 *                          maxiter=, M=) (scipy/sparse/linalg/_isolve/iterative.py:582-841)
 * The config/entry layer the reference does have (XML node lookups, ini_info.py:72-118;
 * step objects with main(), hypervisor.py:589-594) is mirrored in Python by
 * vt-precondition_amd/vtconfig + vtsetup, which call this ABI through ctypes.
 *
 * Conventions: every int-returning function returns VTK_OK (0) or a negative vtk_status;
 * nothing throws or aborts across the boundary; vtk_last_error() explains the last failure
 * of a context (vtk_last_error(NULL, ...) the last failure of a context-free call).
 * Handles are opaque, owned by the caller, freed by the matching *_destroy.  Host arrays
 * passed in stay owned by the caller (they are copied).  A handle is not thread-safe:
 * one context per thread and device, one rank per process.
 */
#ifndef VTKRYLOV_H
#define VTKRYLOV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTK_ABI_VERSION 6   /* 6: VTK_ERR_PEER, vtk_precond_matvec */

typedef struct vtk_ctx vtk_ctx;
typedef struct vtk_csr vtk_csr;
typedef struct vtk_prec vtk_prec;

typedef enum {
    VTK_OK = 0,
    VTK_ERR_ARG = -1,       /* bad argument / shape / index                        */
    VTK_ERR_HIP = -2,       /* HIP runtime error                                   */
    VTK_ERR_RCCL = -3,      /* RCCL error                                          */
    VTK_ERR_SINGULAR = -4,  /* singular diagonal block (numpy.linalg.LinAlgError)  */
    VTK_ERR_NOMEM = -5,     /* host or device allocation failed                    */
    VTK_ERR_STATE = -6,     /* call not valid in this state (e.g. comm not set)    */
    VTK_ERR_NODEVICE = -7,  /* no HIP device: the product has no CPU fallback      */
    VTK_ERR_PEER = -8       /* another rank failed mid-solve; this rank left the   */
                            /* solve at the same Arnoldi step (vtk_gmres)          */
} vtk_status;

typedef enum { VTK_PTR_HOST = 0, VTK_PTR_DEVICE = 1 } vtk_ptr_kind;

typedef enum {
    VTK_ORTH_MGS = 0,   /* modified Gram-Schmidt, SciPy's sequence (iterative.py:755-759):
                           j+2 dependent reductions per Arnoldi step                        */
    VTK_ORTH_DCGS2 = 1, /* delayed classical GS with re-orthogonalisation: ONE reduction and
                           two passes over the basis per step; restart <= 32                */
    VTK_ORTH_AUTO = 2   /* default: DCGS2 when restart <= 32, else MGS (stats.orth reports) */
} vtk_orth;

/* How the block-Jacobi preconditioner is applied (same M^-1 either way):                   */
typedef enum {
    VTK_BJ_AUTO = 0,    /* default: TRIDIAG when available, else INVERSE                      */
    VTK_BJ_INVERSE = 1, /* z_b = inv_b r_b, serial row dots: bit-identical to the oracle      */
    VTK_BJ_TRIDIAG = 2  /* every diagonal block tridiagonal (bs 2/4/8): LU factors, 24 B/row
                           instead of 8 bs B/row; equal to INVERSE to rounding (factors are
                           checked against the inverse to 1e-10 at setup)                    */
} vtk_bj_mode;

/* Device layout of a CSR operator's SpMV (results are bit-identical in both: every row is
 * summed serially in stored order, as csr_matvec does):                                     */
typedef enum {
    VTK_LAYOUT_AUTO = 0, /* default: SELL when its padding is <= 25 % of nnz, else CSR        */
    VTK_LAYOUT_CSR = 1,  /* CSR-stream tiles (products staged in LDS, one lane per row)       */
    VTK_LAYOUT_SELL = 2, /* SELL-64 copy: one wavefront per 64 rows, entries column-major;
                          * columns dictionary-coded per 64-row chunk (4-bit codes into the
                          * chunk's <= 15 distinct col-row offsets; chunks with more keep int32) */
    VTK_LAYOUT_SELL32 = 3 /* SELL-64 with int32 columns everywhere                              */
} vtk_layout;

/* what vtk_csr_layout_info reports: the layout in use and the bytes one SpMV reads of the
 * operator in it (values, columns or codes + dictionaries, offsets)                          */
typedef struct {
    int layout;              /* vtk_layout in use (never AUTO)                                */
    double matrix_bytes;
    int64_t sell_chunks, sell_entries, wide_chunks;
} vtk_layout_info;

/* Synthetic Vlasov operator parameters. */
typedef struct {
    int dim;            /* 1, 2 or 4                                   */
    int fp32;           /* 1: values stored as float32 (C4)            */
    int64_t shape[4];   /* (n) | (Nx, Nv) | (Nx, Ny, Nvx, Nvy)          */
    double vmax, E0, nu, alpha, cfl;
} vtk_vlasov_params;

typedef struct {
    int64_t inner_iters;   /* Arnoldi steps over all restart cycles (SciPy's inner_iter)  */
    int64_t restarts;      /* restart cycles run                                          */
    double presid;         /* last preconditioned residual estimate                       */
    double rnorm;          /* last true residual ||b - A x||                              */
    double bnorm;          /* ||b||                                                       */
    double atol_eff;       /* max(atol, rtol*||b||)  (_get_atol_rtol, iterative.py:19)    */
    double t_solve;        /* seconds, device work of the solve (host wall, synced)       */
    double bytes_moved;    /* algorithmic HBM bytes of the solve           */
    int breakdown;         /* 1 if the last cycle hit h1 <= eps*h0                        */
    int orth;              /* vtk_orth used                                               */
    int band;              /* 1: the line-band DCGS2 step ran (vtk_csr_set_line_band)      */
} vtk_stats;

/* ---- library ------------------------------------------------------------------------ */
int vtk_abi_version(void);
/* 16 hex digits: SHA-256 of the library's sources (the .hip, .hpp and .cpp files of csrc, this
 * header, the Makefile and its EXTRA flags) at build time.  Callers that ship a prebuilt binary next to the
 * sources (the GPU box) compare it with the checked-out tree (vtkrylov._abi.check_build_id).
 * (ABI 5) */
const char *vtk_build_id(void);
const char *vtk_status_string(int status);
/* last error message of ctx (or of the last context-free call when ctx == NULL) */
int vtk_last_error(vtk_ctx *ctx, char *buf, size_t len);

/* ---- host-only helpers (no GPU required) -------------------------------------------- */
/* operator assembly (Appendix A) */
int vtk_vlasov_size(const vtk_vlasov_params *p, int64_t *n, int64_t *nnz);
/* rows [r0, r1): indptr has r1-r0+1 entries starting at 0; indices are global columns;
 * data is double[] or float[] per p->fp32; buffers sized for the row block's nnz */
int vtk_vlasov_generate(const vtk_vlasov_params *p, int64_t r0, int64_t r1, int32_t *indptr,
                        int32_t *indices, void *data);
/* b[i - r0] = 2 * ((splitmix64(seed + i) >> 11) * 2^-53) - 1   */
int vtk_rhs_splitmix(uint64_t seed, int64_t r0, int64_t r1, double *b);
/* contiguous row partition: offsets[world+1], boundaries multiples of align, balanced by
 * nnz when indptr (global, n+1 entries) is given, else by rows */
int vtk_partition_rows(int64_t n, const int32_t *indptr, int world, int align, int64_t *offsets);
/* Halo plan of one rank's row block.  In: local CSR with GLOBAL column
 * indices, the partition offsets.  Out: local_indices (nnz entries; owned column c ->
 * c - row_begin, halo column -> n_local + position in halo_cols), halo_cols (global ids,
 * sorted ascending, so grouped by owner rank) and halo_count_per_rank[world].  Pass
 * halo_cols == NULL to query *n_halo first. */
int vtk_halo_plan(int64_t n_global, const int64_t *offsets, int world, int rank,
                  int64_t nnz, const int32_t *indices, int32_t *local_indices,
                  int64_t *n_halo, int64_t *halo_cols, int64_t *halo_count_per_rank);

/* Geometry of the line-band DCGS2 step (vtk_csr_set_line_band) for a slab of
 * n_local rows in lines of line_len rows on a device with n_cu compute units (n_cu <= 0: 256).
 * VTK_ERR_ARG when the step cannot run on such a slab: line_len not a multiple of 8, n_local
 * not whole lines, fewer than 2 lines, or a slab (with its two halo lines) beyond the kernels'
 * 32-bit row / column indices.  (ABI 3) */
typedef struct {
    int parts;          /* wavefronts per line, <= 56 rows each (> 1 needs couplings within v-1..v+1) */
    int wg_per_range;   /* workgroups per line range */
    int waves_per_wg;   /* wavefronts per workgroup (<= 8: two per SIMD) */
    int ranges;         /* line ranges of one launch; every range walks its lines in order */
    int64_t lines;      /* lines of the slab */
} vtk_band_geometry;
int vtk_line_band_plan(int64_t n_local, int64_t line_len, int n_cu, vtk_band_geometry *out);

/* ---- device context / communicator ---------------------------------------------------- */
int vtk_device_count(int *count);
int vtk_ctx_create(int hip_device, vtk_ctx **out);      /* owns one hipStream_t */
void vtk_ctx_destroy(vtk_ctx *ctx);
int vtk_ctx_stream(vtk_ctx *ctx, void **hip_stream);    /* the stream all work runs on */
int vtk_ctx_synchronize(vtk_ctx *ctx);
/* Tuning switches of a context.  Defaults are the production path; the other
 * settings exist for in-process A/B measurements and for the bit-identity tests (the same sums
 * with and without a byte-saving form).  Each key is seeded from the environment variable
 * VTK_<KEY in upper case> once, when the context is created; the library reads its environment
 * nowhere else (fail_step is a test hook: this rank fails its DCGS2 step of that index in the
 * first cycle, vtk_gmres).  Keys: band, band_lsv, sell_canon, band_canon, band_opt, band_long_rows, lsv_ring,
 * prof_perj, comm_solo, auto_band, grid4, c4_fused, g4_ring, g4_gr, g4_fast, line_fuse, cyc_ring,
 * line2_dc, bcg_fuse, linec_serial, neu_fuse, neu_dc, fail_step.
 * VTK_ERR_ARG for an unknown key; a VTK_<KEY> variable of a key removed in round 5 draws a
 * warning on stderr at context creation and is otherwise ignored.  (ABI 5; fail_step ABI 6;
 * band_long_rows round 6: band_opt bits 3 and 4 only on ranks of at least that many rows;
 * band_opt bit 5, odd band steps walking their line ranges the other way round, at every size;
 * band_opt bit 6 (64), the band step and step 0 of its cycle without the read of the operator's
 * diagonal: w = p + M^-1 (A - M) p, valid because the band step runs only with the tridiagonal
 * block-Jacobi factors of the operator's current values -- last-bit differences in w, default on;
 * bcg_fuse: vtk_bicgstab forms phat = M p and shat = M s inside its vector kernels for block Jacobi
 * with bs in {1, 2, 4, 8} -- 0: the separate apply, the same bits) */
int vtk_ctx_set_tuning(vtk_ctx *ctx, const char *key, int value);
int vtk_ctx_get_tuning(vtk_ctx *ctx, const char *key, int *value);
/* rank 0 creates the 128-byte RCCL unique id; the caller broadcasts it (any transport) */
int vtk_comm_unique_id(void *out128);
int vtk_comm_init(vtk_ctx *ctx, int rank, int world, const void *rccl_unique_id);
/* Host-staged communicator (test/debug transport, e.g. several ranks sharing one GPU, which
 * RCCL refuses): the library synchronises its stream, copies the payload to host memory, calls
 * these hooks and copies the result back.  Counts and offsets are in elements.  Each hook
 * returns 0 on success.  The production path is RCCL (vtk_comm_init). */
typedef struct {
    void *user;
    int (*allreduce_sum_f64)(void *user, double *buf, int64_t count);
    int (*alltoallv)(void *user, const void *sendbuf, const int64_t *send_counts,
                     const int64_t *send_offsets, void *recvbuf, const int64_t *recv_counts,
                     const int64_t *recv_offsets, int64_t elem_bytes);
    int (*allgather)(void *user, const void *sendbuf, void *recvbuf, int64_t bytes_per_rank);
} vtk_host_comm;
int vtk_comm_init_host(vtk_ctx *ctx, int rank, int world, const vtk_host_comm *ops);
int vtk_comm_info(vtk_ctx *ctx, int *rank, int *world);
/* ranks of the context's RCCL communicator (ncclCommCount); 0 when the context has none
 * (world 1, or the host-staged transport) */
int vtk_comm_rccl_count(vtk_ctx *ctx, int *count);

/* ---- operator ------------------------------------------------------------------------ */
/* Row block [offsets[rank], offsets[rank+1]) of an n_global x n_global CSR matrix with
 * GLOBAL column indices.  offsets has world+1 entries (NULL when world == 1).  Arrays are
 * host or device memory per ptr_kind and are copied. */
int vtk_csr_create(vtk_ctx *ctx, int64_t n_global, const int64_t *offsets, int64_t nnz_local,
                   const int32_t *indptr, const int32_t *indices, const void *data,
                   int data_is_fp32, int ptr_kind, vtk_csr **out);
/* generate this rank's rows of the Vlasov operator directly into device memory */
int vtk_csr_create_vlasov(vtk_ctx *ctx, const vtk_vlasov_params *p, const int64_t *offsets,
                          vtk_csr **out);
int vtk_csr_info(vtk_csr *A, int64_t *n_global, int64_t *row_begin, int64_t *row_end,
                 int64_t *nnz_local, int64_t *n_halo);
/* copy this rank's CSR back (indices GLOBAL), host memory */
int vtk_csr_download(vtk_csr *A, int32_t *indptr, int32_t *indices, void *data);
void vtk_csr_destroy(vtk_csr *A);
/* ---- value updates (time stepping: same sparsity pattern, new values every step) ----------
 * SciPy statement: A.data[:] = new_values.  After a successful update A is indistinguishable
 * from an operator freshly created with those values on the same context, tuning and layout
 * (download, SpMV bits in every layout, line values / 4D grid tables -- rebuilt and re-checked,
 * dropped when the new values no longer pass, regained when they pass again --, the kernels
 * vtk_gmres picks and its result bits); everything planned from the pattern (halo plan, tiles,
 * SELL offsets and codes, band layout) is kept.  Every allocation precedes the first overwrite:
 * a VTK_ERR_ARG or VTK_ERR_NOMEM return leaves A as it was.  The work runs on the context's
 * stream.  A preconditioner built before the update keeps its old factors until
 * vtk_prec_refresh: solving with such a lagged M is legal.  A lagged block-Jacobi M applies its
 * inverse rows whatever its mode (the tridiagonal apply of the SELL kernels takes the blocks'
 * off-diagonals from A's rows, which are no longer the values M was factored from);
 * vtk_bjacobi_get_mode reports INVERSE until the refresh.  (additive, ABI 6)
 *
 * Replace the values of A, keeping its sparsity pattern.  data: nnz_local values in the
 * order of vtk_csr_create / vtk_csr_download, float when A was created with fp32 values,
 * else double; host or device per ptr_kind; copied.  Rank-local, no collective. */
int vtk_csr_update_values(vtk_csr *A, const void *data, int ptr_kind);
/* The same for an operator made by vtk_csr_create_vlasov: regenerate this rank's values
 * from p on the device.  dim, shape and fp32 must equal the creating parameters
 * (VTK_ERR_ARG otherwise; VTK_ERR_STATE for an operator not created that way);
 * vmax, E0, nu, alpha, cfl may change. */
int vtk_csr_update_vlasov(vtk_csr *A, const vtk_vlasov_params *p);
/* Number of successful value updates of A (0 after creation). */
int vtk_csr_values_epoch(vtk_csr *A, int64_t *epoch);
/* choose the SpMV layout (vtk_layout); SELL builds the copy on first use (device memory:
 * 12 B per padded entry, 8 B with f32 values) */
int vtk_csr_set_layout(vtk_csr *A, int layout);
int vtk_csr_get_layout(vtk_csr *A, int *layout_in_use);
int vtk_csr_layout_info(vtk_csr *A, vtk_layout_info *out);
/* Line-band structure: rows form x-lines of `line_len` consecutive rows and
 * every column lies in the lines x-1, x, x+1 (mod n / line_len) of its row's line x -- the 2D
 * Vlasov operators with line_len = Nv (set automatically by vtk_csr_create_vlasov, on one rank
 * or across ranks).  Checked on the device (VTK_ERR_ARG when the structure does not hold;
 * line_len 0 clears it; the local row count and its halo must fit 32-bit indices).  Across
 * ranks (world > 1) the call is collective: each rank's slab must hold whole lines with the two
 * neighbour lines as its halo, and the band is set on every rank or on none.  With it,
 * vtk_gmres runs each DCGS2 update pass together with the next step's SpMV + BJ + dots in one
 * sweep (SELL layout, tridiagonal BJ(8), restart <= 20; across ranks the neighbours' edge lines
 * of v_{j-1} and w_j travel as ghost lines each step): the basis is read once per Arnoldi step
 * instead of twice, and the candidate p_j is recomputed in registers instead of stored.
 * Same operator, same update arithmetic. */
int vtk_csr_set_line_band(vtk_csr *A, int64_t line_len);
int vtk_csr_get_line_band(vtk_csr *A, int64_t *line_len);
/* *separable = 1 when the line band is set and the operator's values are line-separable: every
 * coupling to line x+-1 depends only on the position v in the line, every coupling to v+-1 in
 * the same line only on the line x (the 2D Vlasov operators: advection in x with speed v, force
 * along v with field E(x)).  Checked bit for bit against the CSR when the band is set; the band
 * step then reads the diagonal per row and those couplings from per-position / per-line tables
 * (8 B of values per row instead of 40; the same values, summed in the same order).  2: also
 * every row canonical (the couplings to x-1, v-1, the diagonal, v+1, x+1 in ascending column
 * order): the band step derives the entries' kinds and order from the row's line and reads no
 * column codes either.  ABI 4. */
int vtk_csr_get_line_values(vtk_csr *A, int *separable);
/* 4D phase-space grid: rows ((ix Ny + iy) Nvx + jvx) Nvy + jvy, x and y periodic,
 * vx and vy Dirichlet, every row coupled to x+-1, y+-1, vx+-1, vy+-1 in ascending column order,
 * each coupling's value depending on one coordinate (x: jvx, y: jvy, vx: ix, vy: iy) -- the 4D
 * Vlasov operators.  Checked on the device bit for bit (VTK_ERR_ARG when it does not hold; Ny 0
 * clears it); set automatically by vtk_csr_create_vlasov (dim 4) and by vtk_csr_create when the
 * first row's column distances are 1, Nvy, Nvx Nvy, Ny Nvx Nvy.  With it the solver's SpMV
 * launches take each row's columns from its coordinates and its values from the diagonal per row
 * and per-coordinate tables (one value per row read instead of nine values and nine codes; the
 * same sums).  Rank-local, not collective; across ranks the slabs must be whole x planes with the
 * two neighbour planes as the halo.  dims = {Ny, Nvx, Nvy} (zeros: not set).  (ABI 5) */
int vtk_csr_set_grid4(vtk_csr *A, int64_t Ny, int64_t Nvx, int64_t Nvy);
int vtk_csr_get_grid4(vtk_csr *A, int64_t *dims);

/* y = A x on this rank's rows; x holds this rank's rows of the vector (halo exchanged
 * internally over RCCL when world > 1).  Bit-identical to csr_matvec (serial row sums). */
int vtk_spmv(vtk_csr *A, const double *x, double *y, int ptr_kind);

/* ---- block-Jacobi preconditioner ------------------------------------------------------- */
int vtk_bjacobi_create(vtk_csr *A, int block_size, vtk_prec **out);
/* how the block inverses are computed: EXACT = Gauss-Jordan with partial pivoting, one lane per
 * block row, bit-identical to numpy.linalg.inv's oracle restatement; MFMA (bs 16 / 32 only) =
 * blocked Gauss-Jordan whose rank-4 panel updates run on v_mfma_f64_16x16x4f64 -- the same pivot
 * rule, rounding-level differences; AUTO = MFMA for bs 16 and 32 (2.3x / 4.7x
 * faster at C3), EXACT otherwise.  vtk_bjacobi_create uses EXACT. */
typedef enum { VTK_BJ_SETUP_EXACT = 0, VTK_BJ_SETUP_MFMA = 1, VTK_BJ_SETUP_AUTO = 2 } vtk_bj_setup;
int vtk_bjacobi_create_ex(vtk_csr *A, int block_size, int setup, vtk_prec **out);
/* export the block inverses: (n_local + bs - 1) / bs blocks of bs*bs doubles, row-major */
int vtk_bjacobi_inverse(vtk_prec *M, double *inv, int ptr_kind);
int vtk_bjacobi_apply(vtk_prec *M, const double *r, double *z, int ptr_kind);
/* select the apply (vtk_bj_mode) for vtk_bjacobi_apply and vtk_gmres; VTK_ERR_ARG if TRIDIAG
 * is asked for blocks that are not tridiagonal (or whose factors failed the check) */
int vtk_bjacobi_set_mode(vtk_prec *M, int mode);
/* *mode_in_use = VTK_BJ_INVERSE or VTK_BJ_TRIDIAG; *tridiag_available = 0/1 (either may be NULL) */
int vtk_bjacobi_get_mode(vtk_prec *M, int *mode_in_use, int *tridiag_available);
void vtk_prec_destroy(vtk_prec *M);

/* ---- line-Jacobi preconditioner --------------------------------------
 * Line-implicit x-direction preconditioner.  M keeps A's diagonal and the couplings between
 * global rows R and R +- stride whose line index R / stride lies in the same segment of `seg`
 * consecutive line indices (segments also end at the rank's row block): every (segment,
 * R mod stride) is a tridiagonal system along an x-line, factored by Thomas (no pivoting) and
 * applied by a forward and a backward sweep (24 B of factors per row).  SciPy statement:
 * splu(M).solve as a LinearOperator.  Vlasov operators: stride 1 (1D), Nv (2D), Ny*Nvx*Nvy
 * (4D); seg dividing Nx / world makes M independent of the rank count.  VTK_ERR_SINGULAR
 * when a pivot is zero or not finite.  Apply with vtk_prec_apply (or vtk_bjacobi_apply); use
 * as vtk_gmres's M. */
typedef enum { VTK_PREC_BJACOBI = 0, VTK_PREC_LINE = 1, VTK_PREC_LINE2 = 2, VTK_PREC_LINEC = 3, VTK_PREC_NEUMANN = 4 } vtk_prec_kind;
int vtk_linejacobi_create(vtk_csr *A, int64_t stride, int64_t seg, vtk_prec **out);
/* export the factors l | m | g (3 * n_local doubles; the oracle's orc_line_setup layout) */
int vtk_linejacobi_factors(vtk_prec *M, double *f, int ptr_kind);
/* COMPACT apply (default when available): when every line's x-couplings are bit-equal along
 * the line (x-invariant advection, as in the Vlasov operators, checked at setup) the apply
 * forms l and g from them and reads only m: 16 B/row instead of 32, same result bits.
 * set_compact(0) forces the stored-factor apply; set_compact(1) fails when unavailable. */
int vtk_linejacobi_set_compact(vtk_prec *M, int on);
int vtk_linejacobi_get_compact(vtk_prec *M, int *in_use, int *available);
/* ---- line product: two line directions ----------------------------------
 * M = M1 D^-1 M2 = D + X + Y + X D^-1 Y, the approximate-factorisation (ADI-type) product of two
 * line-Jacobi matrices of A: M_i is exactly vtk_linejacobi_create(A, stride_i, seg_i)'s matrix
 * (the same kept couplings, cuts and Thomas factors), D[r] the sum of row r's stored diagonal
 * entries, X and Y the off-diagonal parts of M1 and M2.  Apply: t = M1^-1 r, u = D .* t (one
 * multiply per row), z = M2^-1 u -- bit-identical to the oracle's
 * line_apply(lf2, D * line_apply(lf1, r)).  SciPy statement:
 * LinearOperator(matvec=lambda r: lu2.solve(D * lu1.solve(r))) with lu_i = splu(M_i).
 * 4D Vlasov operators: strides Ny*Nvx*Nvy (x) and Nvx*Nvy (y).  Both sweeps are rank-local.
 * Argument checks per direction as vtk_linejacobi_create; VTK_ERR_SINGULAR when a pivot of
 * either direction is zero or not finite (the smaller row is reported).  Apply, refresh and
 * destroy through vtk_prec_apply / vtk_prec_refresh / vtk_prec_destroy; usable as vtk_gmres's
 * and vtk_bicgstab's M and in vtk_precond_matvec.  The vtk_linejacobi_* calls refuse it
 * (VTK_ERR_STATE).  Tuning key line2_dc (default 1): the DCGS2 step's dots fused behind the
 * second sweep; 0: the plain second sweep, then the dots kernel.  (additive, ABI 6) */
int vtk_lineproduct_create(vtk_csr *A, int64_t stride1, int64_t seg1, int64_t stride2, int64_t seg2,
                           vtk_prec **out);
/* which 0 / 1: the factors l | m | g of that direction (3 * n_local doubles); 2: D (n_local) */
int vtk_lineproduct_factors(vtk_prec *M, int which, double *f, int ptr_kind);
/* ---- periodic whole lines: cyclic x-line solves -----------------------------
 * M keeps A's diagonal (per row the sum of its stored diagonal entries, in stored order) and every
 * stored coupling between rows R and R' with R mod stride == R' mod stride, R / (stride period) ==
 * R' / (stride period) and line indices (R / stride) mod period that differ by +-1 modulo period:
 * each (block, R mod stride) is one cyclic tridiagonal system of `period` unknowns, the wrap
 * coupling included.  SciPy statement: LinearOperator(matvec=splu(M).solve).  Vlasov operators:
 * (stride, period) = (Nv, Nx) in 2D, (Ny Nvx Nvy, Nx) for the 4D x-lines, (Nvx Nvy, Ny) for the 4D
 * y-lines.  `seg` is only the partition length of the solver, a recursive Schur complement on
 * separators (segments of seg unknowns, one separator each; the separators' system is partitioned
 * again until a level has at most `linec_serial` unknowns per line -- tuning key, default 64, read
 * here -- which one lane per line solves).  It does not change M; the result is defined to
 * rounding, not bit for bit.  No pivoting, at any level (as vtk_linejacobi_create).
 * VTK_ERR_ARG unless period >= 3, seg >= 2, stride >= 1 and the rank's first row and row count are
 * multiples of stride * period (every cyclic line on one rank: the 2D operators across ranks are
 * refused).  VTK_ERR_SINGULAR when a pivot of any level is zero or not finite; the message names
 * the row.  Apply, refresh (every level refactored; M invalid after a failed one) and destroy
 * through vtk_prec_apply / vtk_prec_refresh / vtk_prec_destroy; usable as vtk_gmres's and
 * vtk_bicgstab's M and in vtk_precond_matvec.  The vtk_linejacobi_* and vtk_lineproduct_* calls
 * refuse it (VTK_ERR_STATE).  (additive, ABI 6) */
int vtk_linecyclic_create(vtk_csr *A, int64_t stride, int64_t period, int64_t seg, vtk_prec **out);
/* the partition: levels (the last one is the serial level), unknowns per line and level, whether
 * the spikes are kept as one table per line (compact; 0: stored per row) */
typedef struct {
    int32_t levels;
    int32_t compact;
    int64_t stride, period, seg;
    int64_t unknowns[32];
} vtk_linec_info;
int vtk_linecyclic_info(vtk_prec *M, vtk_linec_info *out);
/* ---- periodic whole lines that span the ranks --------------------------------
 * The same M as vtk_linecyclic_create for ONE block of lines, n_global == stride * period (the 2D
 * x-lines, the 4D x-lines), when the row partition cuts the lines: rank p owns a contiguous range
 * of P_p >= 3 line indices of every line (first row and row count multiples of stride).  `period`
 * is the global one.  SPIKE over ranks on top of the solver above: each rank factors the open
 * chunk of its P_p unknowns per line (the first row's coupling a_first to the previous rank's last
 * row and the last row's c_last to the next rank's first row left out -- both are read from the
 * CSR's halo columns, summed in stored order from 0.0 like every coefficient), keeps
 * V_p = M_p^-1 (a_first e_first) and W_p = M_p^-1 (c_last e_last) (16 B per row), and every rank
 * holds all ranks' spike tips.  An apply solves the chunk, gathers two edge values per line and
 * rank (ONE all-gather of 16 * stride bytes per rank), solves the ranks' interface system per line
 * (redundantly on every rank, no pivoting) and corrects x_p = y_p - V_p xi - W_p eta in the last
 * sweep.  The result is defined to rounding.  With one rank the same path runs with world 1 (it
 * does not delegate to vtk_linecyclic_create).  At most 16 ranks.
 * Creation and vtk_prec_refresh are COLLECTIVE, and every rank returns the same class of status:
 * VTK_ERR_ARG when n_global != stride * period, when a rank's slab is not whole line indices or has
 * fewer than 3 (decided from an all-gather of the local counts), period < 3, seg < 2, stride < 1;
 * VTK_ERR_SINGULAR when any rank's chunk has a zero or non-finite pivot (that rank's message names
 * the row, the others name the rank) or the interface system has one (the message names the line).
 * Any other failure of one rank in its own part (an allocation, a launch) is gathered too: that rank
 * returns its error, the others VTK_ERR_PEER, and none is left in a collective; a collective that
 * itself fails returns at once.
 * Kind VTK_PREC_LINEC; vtk_linecyclic_info reports the levels of the rank's chunk (unknowns[0] =
 * P_p) and the global period.  Usable wherever vtk_linecyclic_create's result is -- vtk_prec_apply,
 * vtk_gmres, vtk_bicgstab, vtk_precond_matvec; every rank must make the same calls -- except as the
 * base of vtk_neumann_create (VTK_ERR_ARG: out of scope).  The vtk_linejacobi_* and
 * vtk_lineproduct_* calls refuse it (VTK_ERR_STATE).  vtk_linecyclic_create itself keeps refusing
 * lines that span ranks.  (additive, ABI 6) */
int vtk_linecyclic_create_span(vtk_csr *A, int64_t stride, int64_t period, int64_t seg, vtk_prec **out);
typedef struct {
    int32_t world, rank;   /* the ranks the lines span, this rank */
    int32_t spanning;      /* 1 */
    int32_t reserved;
    int64_t first_line;    /* the rank's first line index */
    int64_t local_period;  /* P_p: its line indices */
    int64_t period;        /* the global period */
} vtk_linec_span_info;
/* VTK_ERR_STATE for a preconditioner that does not span (vtk_linecyclic_create's included) */
int vtk_linecyclic_span_info(vtk_prec *M, vtk_linec_span_info *out);
/* ---- Neumann-series (polynomial) wrapper around any preconditioner above --------
 * N_k^-1 r:  z_1 = M^-1 r;  z_{i+1} = z_i + M^-1 (r - A z_i), i = 1 .. k-1, with k = degree and
 * M = M_base: the degree-(k-1) Neumann series of M^-1 A, equal to k steps of preconditioned
 * Richardson from 0; N_k^-1 = (I - (I - M^-1 A)^k) A^-1.  More operator work per Krylov vector, so a
 * solve needs fewer Krylov vectors.  SciPy statement:
 *     def mv(r):
 *         z = M(r)
 *         for _ in range(degree - 1):
 *             z = z + M(r - A @ z)
 *         return z
 *     LinearOperator((n, n), matvec=mv)
 * The series helps only while the eigenvalues of M^-1 A stay inside the unit disc around 1: with
 * block Jacobi on the Vlasov operators degree 2 halves the iterations and degree 3 stalls GMRES(20);
 * the line product takes every degree (CPU table).  Nothing selects the wrapper by
 * default.
 * Bit-level definition (the library is compiled with -ffp-contract=off): t = r - (A z), the SpMV's
 * row sum rounded to double, then one subtraction; u = M^-1 t, exactly the base's apply; z + u, one
 * addition per row.  With block Jacobi (either apply mode), line Jacobi and the line product the
 * result equals the composition of vtk_spmv and vtk_prec_apply with those two operations, bit for
 * bit, whichever kernels run it (one fused launch per correction for block Jacobi with bs 1, 2, 4, 8
 * on fused tiles -- tuning neu_fuse --, the addition inside the base's last sweep for the line kinds);
 * with the periodic lines to rounding, as that base is defined.  degree = 1 is the base, bit for bit.
 * 1 <= degree <= 8 (VTK_ERR_ARG).  The wrapper BORROWS its base: the base must outlive every use of
 * the wrapper -- a use after the base's vtk_prec_destroy returns VTK_ERR_STATE -- and destroying the
 * wrapper leaves the base alone.  VTK_ERR_ARG for a base that is itself a wrapper or was built on
 * another operator.  vtk_prec_refresh on the wrapper refreshes the base (its errors pass through,
 * VTK_ERR_SINGULAR with the base's row included); the wrapper's epoch is the base's, and a base
 * refreshed or lagging on its own is seen by the wrapper at its next use.  Apply and destroy through
 * vtk_prec_apply / vtk_prec_destroy; usable as vtk_gmres's and vtk_bicgstab's M and in
 * vtk_precond_matvec, on one rank and across ranks (every correction exchanges its halo).  The
 * line-band DCGS2 step is not taken with it.  The kind-specific vtk_bjacobi_*, vtk_linejacobi_*,
 * vtk_lineproduct_* and vtk_linecyclic_* calls refuse it (VTK_ERR_STATE).  Device memory: three
 * vectors of n_local doubles.  Tuning key neu_dc (default 1): in a DCGS2 step the last correction's
 * addition also leaves the step's dots (line Jacobi and line product with segments <= 32, and the
 * plain addition); 0: the dots kernel follows.  (additive, ABI 6) */
int vtk_neumann_create(vtk_csr *A, vtk_prec *M_base, int degree, vtk_prec **out);
typedef struct {
    int32_t degree;
    int32_t base_kind;   /* vtk_prec_kind of the base */
    int32_t fused;       /* 1: each correction is one SpMV launch with the base in its epilogue */
    int32_t base_alive;  /* 0: the base has been destroyed (every use returns VTK_ERR_STATE) */
} vtk_neu_info;
int vtk_neumann_info(vtk_prec *M, vtk_neu_info *out);
/* z = M^-1 r for any preconditioner; *kind = vtk_prec_kind */
int vtk_prec_apply(vtk_prec *M, const double *r, double *z, int ptr_kind);
int vtk_prec_kind_of(vtk_prec *M, int *kind);
/* Recompute M (BJ, line Jacobi or line product: both directions and D) from its operator's current values into the storage
 * it already owns.  *epoch (nullable) = the operator epoch M now corresponds to.
 * Block Jacobi: the setup M was created with (EXACT or MFMA), the tridiagonal check and the
 * remembered vtk_bjacobi_set_mode request again; VTK_ERR_ARG when an explicit TRIDIAG request
 * can no longer be met (M is refreshed and usable in INVERSE mode).  Line Jacobi: the factors
 * and the x-invariance check again (COMPACT dropped or regained; a set_compact(0) request is
 * kept).  VTK_ERR_SINGULAR as at creation: M is then invalid -- apply, export and vtk_gmres
 * with it return VTK_ERR_STATE -- until a later refresh succeeds.  (additive, ABI 6) */
int vtk_prec_refresh(vtk_prec *M, int64_t *epoch);
/* w = M^-1 (A x): the preconditioned operator GMRES applies at every Arnoldi step (SciPy:
 * M.matvec(A @ x), iterative.py:752), computed by the launch the solver's split DCGS2 step uses
 * for this operator and preconditioner (the 4D grid-row ring kernel -- across ranks in the
 * solver's interior / boundary form --, else the SpMV with the BJ epilogue, else SpMV then
 * apply); M may be NULL (w = A x).  Bit-identical across those forms, and to vtk_bjacobi_apply
 * of vtk_spmv, with the INVERSE apply: the kernel-level pin.  With the TRIDIAG apply the SELL
 * kernels (and the ring kernel) read m alone and form l_i = sub_i m_{i-1} from the row's own
 * entry where the stored factor is sub_i / u_{i-1}: bit-identical among themselves, equal to the
 * CSR-layout epilogue and to vtk_bjacobi_apply (both solve with the stored l | m | g) to rounding. */
int vtk_precond_matvec(vtk_csr *A, vtk_prec *M, const double *x, double *w, int ptr_kind);

/* ---- solver --------------------------------------------------------------------------- */
/* scipy.sparse.linalg.gmres semantics (iterative.py:582-841, callback=None): restarted,
 * left-preconditioned GMRES(restart); maxiter counts restart cycles (<= 0: 10 n); x holds
 * x0 on entry and the solution on exit; info = 0 on convergence else maxiter.
 * Across ranks (DCGS2): a rank whose launch fails mid-solve returns its error, and every
 * rank -- the failing one included -- leaves the solve after the same Arnoldi step: the
 * failure travels as a vote in the step's all-reduce, so no rank is left blocked in a
 * collective; the peers return VTK_ERR_PEER and the communicator stays usable.  A failed
 * collective itself (VTK_ERR_RCCL) marks the communicator broken: vtk_ctx_destroy then
 * aborts it (ncclCommAbort) instead of destroying it.  (The modelled failure is a launch the
 * rank could not issue; a device fault that kills the HIP context cannot join any collective
 * and is left to the launcher's watchdog.) */
int vtk_gmres(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
              int restart, int64_t maxiter, int ptr_kind, int *info, vtk_stats *stats);
int vtk_gmres_set_orth(vtk_ctx *ctx, int orth);
/* on (default) / off: the line-band DCGS2 step when the operator and preconditioner allow it
 * (vtk_csr_set_line_band); off keeps the separate update pass and fused SpMV step */
int vtk_gmres_set_band(vtk_ctx *ctx, int on);

/* ---- compressed Krylov basis (additive, ABI 6) ---------------------------
 * VTK_BASIS_F32: vtk_gmres stores the orthonormal columns of a restart cycle in float32 and
 * computes in float64 (compressed-basis GMRES).  Off by default; VTK_BASIS_F64 is the solver as
 * it always was -- the same launches, the same bits, no extra allocation.
 *
 * What is rounded, and where.  A cycle keeps the finalised columns v^_0 .. v^_{restart-1} in
 * float32 and two float64 vectors for the candidates p_j and p_{j+1}.  The cycle start scales
 * M^-1 r in float64, stores v^_0 = (float) v_0 and applies the operator to the stored value.
 * The update pass of step j forms v_j = (p_j - V^_j s) / r in float64, stores v^_j = (float) v_j,
 * and subtracts e_j v^_j -- the stored value widened -- from w: p_{j+1} is float64 and orthogonal
 * (to rounding) to the columns every later step reads.  The operator is applied to the float64
 * candidate p_j.  The dots, the projections and the x update x += sum_k y_k v^_k widen the
 * stored columns and accumulate in float64; a column that enters x before it was stored is
 * rounded to float32 the same way first.  w, the residual, the Hessenberg matrix, the Givens
 * rotations and every scalar stay float64, and the true residual is recomputed in float64 at
 * every restart, so the stopping test is the float64 solver's.
 *
 * Results are therefore defined to float32-basis rounding: the stored columns are orthonormal to
 * about 6e-8 instead of 1e-16, x and the iteration count agree with the float64 basis to the
 * solver's tolerance, not bit for bit, and a cycle that alone reduces the residual by about 2^24
 * or more pays an extra cycle.  Runs are deterministic.
 *
 * The option runs on the DCGS2 sequence with the separate dots and update passes: the line-band
 * step is not taken (vtk_stats.band = 0) and no operator step fuses the dots of a step that reads
 * stored columns.  With the MGS sequence (VTK_ORTH_MGS, or VTK_ORTH_AUTO with restart > 32) vtk_gmres
 * returns VTK_ERR_ARG: select DCGS2.  Across ranks every rank must make the same choice; otherwise
 * every rank returns VTK_ERR_ARG.  The capture hook returns the float32 columns widened
 * (VTK_CAP_V), with the candidate still open at cycle end in its column; final_cols keeps its
 * DCGS2 rule. */
typedef enum { VTK_BASIS_F64 = 0, VTK_BASIS_F32 = 1 } vtk_basis;
int vtk_gmres_set_basis(vtk_ctx *ctx, int basis);   /* an unknown value: VTK_ERR_ARG */
typedef struct {
    int32_t requested, used;   /* vtk_basis: set on ctx; used by the last vtk_gmres on ctx       */
    int64_t basis_bytes;       /* that solve's basis: the stored columns and candidate vectors   */
    int64_t workspace_bytes;   /* that solve's whole workspace (basis included)                  */
} vtk_basis_info;
int vtk_gmres_basis_info(vtk_ctx *ctx, vtk_basis_info *out);

/* ---- capture of one restart cycle (a TEST HOOK: off by default, not part of the integration
 * surface; additive, ABI 6) -----------------------------------------------------------------
 * The solver's workspace after a solve does not show a cycle's Arnoldi factorisation: the
 * cycle-end residual writes the next v0 direction into V[0], and a later cycle overwrites
 * everything.  An armed capture copies, device to device on the context's stream, x at the
 * start of the chosen cycle (before the cycle's x update, wherever that runs) and, between the
 * x update and the cycle-end residual, all restart + 1 columns of V, H (rotated), S, giv and,
 * under DCGS2, Hraw (the unrotated Hessenberg columns) and the step coefficients.
 *   cycle >= 0: that 0-based restart cycle of every following vtk_gmres on the context;
 *   cycle == -1 (default): off -- the solve issues no allocation, copy or synchronisation for it;
 *   cycle == -2: every cycle, the last one run is kept.
 * The buffer belongs to the context and is freed with it.  Across ranks each rank captures its
 * own rows; no collective is added.
 *
 * vtk_arnoldi_info.final_cols: the leading columns of V that are FINAL at cycle end, i.e. hold
 * v_0 .. v_{final_cols-1} normalised (and, under DCGS2, re-orthogonalised).  The rule:
 *   MGS: the tail of column c stores v_{c+1}: final_cols = cols + 1 (cols on a breakdown, whose
 *        last vector is stored unnormalised);
 *   DCGS2 (split, fused, ring, line and band steps alike): v_j (j >= 1) is stored by the update
 *        pass of step j, one step after its candidate p_j.  The step whose scalar kernel stops
 *        the cycle (xup_tag = j; the last column of a full cycle stops it at j = restart - 1 when
 *        it commits early) turns its update pass into the x update: V[j] keeps the candidate p_j
 *        -- or, on the band path, which never stores p_j for j <= restart - 2, whatever an earlier
 *        cycle left there -- and v_j enters x recomputed, not as a column of V.
 *        final_cols = max(xup_tag, 1); a cycle closed by the closing reduction (xup_tag < 0)
 *        ran every update pass: final_cols = restart.
 * The Arnoldi relation B v_c = V[:, :c+2] h_c can be checked for c + 1 < final_cols; every such
 * column was finalised exactly (an early commit always stops the cycle at its column).
 * H is column-major with leading dimension restart + 1 (column c at c (restart + 1)), Hraw
 * likewise with restart + 1 columns; h_{c+1,c} of a column committed early is the tentative nu
 * (VTK_CAP_NU), its Hraw rows 0..c the tentative column. */
typedef struct {
    int64_t n_local, ld;   /* rows of this rank; leading dimension of V                    */
    int restart, cycle;    /* m; the cycle captured                                         */
    int cols, final_cols;  /* columns committed to H; final leading columns of V           */
    int orth, band;        /* VTK_ORTH_MGS / VTK_ORTH_DCGS2; 1: the line-band step ran      */
    int has_hraw;          /* 1 under DCGS2                                                 */
    int stop_col, breakdown, xup_tag;   /* the cycle's device record (stop_col >= 2^30: ran out) */
} vtk_arnoldi_info;
enum { VTK_CAP_V = 0,          /* (restart + 1) * ld doubles                                */
       VTK_CAP_X_IN = 1,       /* n_local doubles                                           */
       VTK_CAP_H = 2,          /* restart * (restart + 1) doubles                           */
       VTK_CAP_S = 3,          /* restart + 1                                               */
       VTK_CAP_GIV = 4,        /* 2 restart: c_0 s_0 c_1 s_1 ...                            */
       VTK_CAP_HRAW = 5,       /* (restart + 1)^2 doubles (DCGS2)                           */
       VTK_CAP_COMMITTED = 6,  /* restart + 1 int32 (DCGS2)                                 */
       VTK_CAP_NU = 7 };       /* 1 double: the last tentative h_{j+1,j} (DCGS2)            */
int vtk_gmres_capture(vtk_ctx *ctx, int cycle);
/* VTK_ERR_STATE when nothing is captured: never armed, the chosen cycle not reached, or a later
 * vtk_gmres on the context ran without capture */
int vtk_gmres_captured(vtk_ctx *ctx, vtk_arnoldi_info *info);
int vtk_gmres_captured_read(vtk_ctx *ctx, int what, void *dst, int ptr_kind);

/* scipy.sparse.linalg.bicgstab semantics (iterative.py, bicgstab, callback=None): right-
 * preconditioned BiCGStab, M approximating A^-1 (NULL: none); x holds x0 on entry.  info as
 * SciPy's: 0 converged (||r|| or ||s|| of the recurrence below max(atol, rtol ||b||)), -10 the
 * rho breakdown, -11 the omega or <rtilde, v> breakdown, else maxiter (<= 0: 10 n; at most
 * 2^29 - 3 iterations are run).  x changes only by the iteration's two updates: on a breakdown it
 * holds the last completed iterate.  Fixed memory: seven work vectors of n_local doubles,
 * allocated for the call.  Every test and every scalar of the loop stays on the device; the
 * host issues iterations ahead and watches a mapped stop flag, with no synchronisation per
 * iteration.  (additive, ABI 6)
 *
 * ACROSS RANKS (a context with a communicator, 1-8 ranks): b and x are this rank's rows, as
 * for vtk_gmres; every rank passes the same rtol, atol and maxiter; a rank without rows takes
 * part in every collective.  An iteration has two halo exchanges and four all-reduces of a
 * small record each (the sums a scalar step consumes plus a failure vote); ||b||, the
 * `x0.any()` flag and the true residual are all-reduced too, so the bnrm2 == 0 shortcut and
 * the r = b / r = b - A x0 choice are global decisions and info and every field of the
 * statistics but t_solve are the same on every rank.  Every rank enqueues the same iterations:
 * the host leaves the loop on the device's stop record alone.
 * Failure containment, as for vtk_gmres: a rank whose launch fails mid-solve sets a sticky
 * vote and keeps issuing the same launches and collectives; the first scalar step that reads
 * a nonzero all-reduced vote stops every rank at the same point, and x is never partly
 * updated by the iteration in which the vote arrived.  The failing rank returns its own error
 * (a failed allocation of the work vectors, VTK_ERR_NOMEM, travels in the first all-reduce),
 * the others VTK_ERR_PEER; the communicator stays usable.  A collective that itself fails
 * (VTK_ERR_RCCL, or a host hook) returns at once and marks the communicator broken. */
typedef struct {
    int64_t iterations;    /* v = A M p products computed                          */
    double rnorm;          /* true residual ||b - A x|| of the returned x          */
    double bnorm, atol_eff;
    double t_solve;        /* seconds, as vtk_stats.t_solve                        */
    double bytes_moved;    /* algorithmic bytes, DESIGN.md §4 conventions          */
    int half_step;         /* 1: left through the ||s|| test                       */
} vtk_bicgstab_stats;
int vtk_bicgstab(vtk_csr *A, vtk_prec *M, const double *b, double *x, double rtol, double atol,
                 int64_t maxiter, int ptr_kind, int *info, vtk_bicgstab_stats *stats);

/* ---- kernel profile (measurement) ------------------------------------------
 * When enabled, every kernel the library launches is bracketed by HIP events on the
 * context's stream; per kernel class the driver accumulates launches, device seconds and the
 * ALGORITHMIC bytes of each launch (the per-unit figures of SURVEY.md §8d).  No-op launches
 * after a cycle's stop column are not counted.  Costs ~a few us per launch: not for timing
 * whole solves. */
typedef struct {
    char name[32];       /* kernel class, e.g. "spmv_bj", "mgs", "tail", "spmv"        */
    int64_t launches;
    double seconds;      /* sum of event-measured durations                            */
    double bytes;        /* sum of algorithmic bytes                                   */
} vtk_kernel_profile;
int vtk_profile_enable(vtk_ctx *ctx, int on);   /* on: also clears the counters */
int vtk_profile_read(vtk_ctx *ctx, vtk_kernel_profile *out, int max_entries, int *n_entries);

#ifdef __cplusplus
}
#endif
#endif /* VTKRYLOV_H */
