// vtk_internal.hpp — types shared by the host units (listed in vtk_driver.hpp) and vtk_host.cpp, and the
// gfx950 kernels (vtk_kernels.hip).  Not part of the public ABI.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/vtkrylov.h"

namespace vtk {

// ---- kernel geometry -------------------------------------------------------
constexpr int NT = 256;            // threads per workgroup, every vector kernel
constexpr int TILE_ROWS = 512;     // max rows of one SpMV tile (CSR-stream)
constexpr int TILE_NNZ = 4096;     // max nnz of one stream tile: products staged in LDS (32 KB)
constexpr int GMAX = 1024;         // max workgroups of a reducing kernel = partial-sum slots
constexpr int MAX_RESTART = 1024;  // restart length bound (LDS for y in the x update)
constexpr int BIG_COL = 1 << 30;   // "not stopped" marker of GmresState::stop_col

// ---- device-resident solver scalars ---------------------------------------------------------
struct GmresState {
    double ptol;          // inner tolerance of this cycle (host writes before each cycle)
    double presid;        // |S[col+1]| after the last Givens step
    double rnorm;         // ||b - A x|| (finalise)
    double scal[8];       // misc finalised scalars (bnorm, Mb norm, ...)
    int stop_col;         // column at which the cycle stopped (BIG_COL while running)
    int breakdown;        // h1 <= eps*h0 at stop_col
    long long inner;      // inner iterations, cumulative
    int xup_tag;          // DCGS2: the update pass (step tag) that does the cycle's x update
                          // (-1: none, the host-enqueued k_xupdate does it)
    int pad_;
};

// BiCGStab (vtk_bicgstab; vtk_bicgstab.hip): the scalars of SciPy's loop, kept on
// the device by k_bcg_scalar.  stop is the flag the solve's kernels test: a kernel tagged above it
// returns at entry.  Tags of iteration k: 4k + 1 up to the ||s|| test, 4k + 2 the half-step
// exit's x update (runs only when stop == its tag), 4k + 3 the rest.
struct BicgState {
    double rho, rho_prev, alpha, omega, beta, rv;
    double rnorm, snorm;          // ||r|| and ||s|| of the recurrence (the exit tests)
    long long iterations;         // v = A M p products that count (vtk_bicgstab_stats::iterations)
    int info;                     // SciPy's return code once stopped
    int half_step;                // left through the ||s|| test
    int stop;                     // BCG_RUN while running
    int peer_failed;              // across ranks: an all-reduced failure vote stopped the solve
};
// all-reduced records of the rank path (vtk_ctx::d_scal; the quantities, then the failure vote):
// the pre-loop record | INIT | A | B | omega | C | the true residual; this rank's own sticky vote
// sits at d_scal[DC_VOTE + 1] as in vtk_gmres
enum { BCG_REC_PRE = 8, BCG_REC_INIT = 12, BCG_REC_A = 16, BCG_REC_B = 20, BCG_REC_W = 24, BCG_REC_C = 28,
       BCG_REC_FIN = 32 };
constexpr int BCG_RUN = INT32_MAX;
constexpr int64_t BCG_MAX_ITERS = (INT32_MAX - 8) / 4;   // iterations a solve's tags can number
constexpr int bcg_tag(int64_t k, int part) { return (int)(4 * k + part); }
enum { BCG_PH_INIT = 0, BCG_PH_A = 1, BCG_PH_B = 2, BCG_PH_C = 3 };   // k_bcg_scalar phases

// DCGS2 (delayed classical Gram-Schmidt with re-orthogonalisation, one reduction per Arnoldi
// step): per-step coefficients produced by the scalar kernel for the update pass
constexpr int DC_MAXJ = 32;          // restart <= 32 in this mode (4 waves x 8 vectors per lane)
constexpr int DC_NQ = 2 * DC_MAXJ + 3;   // reduction slots: s[32] | z[32] | alpha beta gamma
// across ranks the all-reduced payload carries one more slot, the failure vote (vtk_ctx::d_scal
// [DC_VOTE]; [DC_VOTE + 1] holds this rank's own vote, nonzero once a launch of it failed)
constexpr int DC_VOTE = DC_NQ;
constexpr int DC_NQV = DC_NQ + 1;
constexpr int PEER_FAILED = 2;           // GmresState::breakdown: the vote stopped the cycle
struct DcCoef {
    double s[DC_MAXJ];        // re-orthogonalisation coefficients of the candidate p_j
    double e[DC_MAXJ + 1];    // projection of w on [V_j, v_j]
    double rinv;              // 1 / r_j  (r_j = ||p_j - V_j s||, Pythagorean)
    double q;                 // 1 / (r_j * nu_{j+1})
    double nu;                // tentative h_{j+1,j}
    double h0[DC_MAXJ + 1];   // ||B v_c|| per column (breakdown test, iterative.py:766)
    int committed[DC_MAXJ + 1];   // column already rotated into H (early or exact commit)
    // the previous step's e and q (k_dc_scalar saves them before overwriting): the line-band
    // step recomputes p_j = (w_{j-1} - sum_k e_prev[k] V_k) q_prev instead of storing it
    double e_prev[DC_MAXJ + 1];
    double q_prev;
};

// a reduced scalar as seen by a consumer kernel: G partials (single GPU) or 1 value (after
// the RCCL all-reduce).  Every consumer workgroup sums the partials in the same fixed order.
struct Red {
    const double *p;
    int cnt;
};

// ---- CSR tiles (CSR-stream row blocks) -----------------------------------------------------
struct Tiles {
    int32_t *d_row = nullptr;   // tile t = rows [row[t], row[t+1])
    int32_t *d_end = nullptr;   // optional (split lists): tile t = rows [row[t], end[t])
    int ntiles = 0;
    int align = 1;              // every boundary is a multiple of align (except n_local)
    bool has_long = false;      // some tile is a single row with nnz > TILE_NNZ
    bool aligned = true;        // no align-group had to be split into single-row tiles
    int grid = 0;               // workgroups of the tile kernels = min(ntiles, GMAX)
    int64_t nrows = 0;          // rows covered (split lists: byte accounting)
};

// SELL-64 copy of a CSR (vtk_kernels.hip k_sell): chunk q = local rows 64q..64q+63
struct Sell {
    int64_t *d_off = nullptr;   // [nch+1] entry offsets (multiples of 64)
    int32_t *d_col = nullptr;   // [entries], -1 = padding
    void *d_val = nullptr;      // [entries] f64 (C4: f32)
    int64_t nch = 0, entries = 0;
    // dictionary-coded columns (k_sell_pack): entry k of row 64q+l is the 4-bit code
    // (pk[pk_off[q] + 64*(k/8) + l] >> 4*(k%8)) & 15; code 15 = padding, else
    // col = row + dict[16q + code].  dict[16q + 15] != 0: the chunk has more than
    // PK_CODES distinct (col - row) offsets and reads d_col instead ("wide")
    uint32_t *d_pk = nullptr;
    int64_t *d_pkoff = nullptr;  // [nch+1] word offsets (multiples of 64)
    int32_t *d_dict = nullptr;   // [nch][16]
    int64_t n_wide = 0;          // chunks that kept int32 columns
    int64_t wide_entries = 0;    // their entries (64 per row slot)
    int64_t pk_words = 0;
    int uniform_w = 0;           // every chunk has this width (offsets are 64 W q): no offset loads
};
constexpr int PK_CODES = 15;     // offsets per chunk dictionary (codes 0..14; 15 = padding)

// groups of 4 SELL chunks (256 rows) a SELL launch covers: all (d_list null) or a list
struct Groups {
    int32_t *d_list = nullptr;
    int count = 0;
    int grid = 0;               // workgroups = min(count, GMAX), >= 1
};

// line-Jacobi operator: the tridiagonal systems along x-lines, cut into
// segments of `seg` consecutive line indices i = R / stride (R global) and at the rank's row
// block [row0, row0 + n).  f = [l | m | g] (n doubles each), Thomas factors (vtk_kernels.hip
// k_line_setup; the oracle's orc_line_setup).  Work items: one wavefront per (segment, 64
// consecutive j = R mod stride starting at j0).
struct LineOp {
    double *f = nullptr;
    int64_t n = 0, row0 = 0, stride = 1, seg = 1;
    int64_t i_lo = 0, i_hi = -1;   // line indices of the block's first / last row
    int64_t nseg = 0;              // segments touching the block
    int64_t j0 = 0, jn = 0;        // lanes cover j = j0 .. j0 + jn - 1
    int64_t jb = 0;                // wavefronts per segment = ceil(jn / 64)
    // compact (x-invariant couplings): a_j = ac[j - j0], c_j = ac[jn + j - j0]; the apply forms
    // l = a m_prev and g = c m and reads only m of f (k_line_setup's ext check)
    double *ac = nullptr;
    int compact = 0;
};

// periodic whole-line operator (vtk_linecyclic_create; vtk_linec.hip): every
// (block, j = R mod stride) of the rank's rows is one cyclic tridiagonal system of `period`
// unknowns, element i of it at local index (block period + i) stride + j.  Level 0 is the lines
// themselves, level k + 1 the separators (one per segment) of level k, in the same layout with
// period = level k's segments per line; the last level has one segment per line.
constexpr int LINEC_MAXLEV = 32;
struct LineCLevel {
    double *f = nullptr;   // l | m | g | V | W (n doubles each): Thomas factors and spikes
    double *x = nullptr;   // levels >= 1: the level's right-hand side, solved in place (n doubles)
    int64_t n = 0, period = 0, seg = 0, nseg = 0;   // unknowns, per line: unknowns, segment length, segments
};
// lines that span the ranks (vtk_linecyclic_create_span): the levels above are those
// of the rank's open chunk of `period` = P_p unknowns per line (one block), the rank level couples
// the chunks: x_p = y_p - V_p xi - W_p eta with xi the previous rank's last unknown and eta the next
// rank's first (cyclically)
constexpr int LINEC_SPAN_MAXW = 16;   // ranks the interface kernel holds in registers
struct LineCSpan {
    bool on = false;
    int world = 1, rank = 0;
    int64_t gperiod = 0, i0 = 0;   // the global period; the rank's first line index
    double *vw = nullptr;          // V_p | W_p (n doubles each)
    int32_t *ecol = nullptr;       // [2][stride] local columns of a_first's / c_last's entries (-1: none)
    double *tsend = nullptr;       // this rank's V_first | V_last | W_first | W_last (stride each) | flag
    double *tips = nullptr;        // [world][4 stride + 1] every rank's, gathered at setup
    double *edge = nullptr;        // this rank's y_first | y_last (stride each), written per apply
    double *edges = nullptr;       // [world][2 stride] every rank's, gathered per apply
    double *xe = nullptr;          // xi | eta of this rank (stride each): the interface solve's result
};
struct LineC {
    int64_t n = 0, row0 = 0, stride = 1, period = 0, seg = 0, nblk = 0;
    int nlev = 0, serial = 64;
    LineCLevel lev[LINEC_MAXLEV];
    double *minv = nullptr;   // [nblk stride] the last level's reciprocal pivots
    LineCSpan sp;
};

// 4D phase-space grid of the Vlasov operators (row = ((ix Ny + iy) Nvx + jvx) Nvy + jvy, x and y
// periodic, vx and vy Dirichlet): every row couples to x +- 1 (value by jvx),
// y +- 1 (by jvy), vx +- 1 (by ix), vy +- 1 (by iy) and itself, in ascending column order.  When
// vtk_csr_set_grid4 / the Vlasov assembly / the drop-in detection verified that (bit for bit),
// the solver's SELL launches take each row's columns from its coordinates and its values from
// D[n] (the stored value type) and the per-coordinate tables: 4 B of matrix per row (C4) instead
// of 9 values and 9 codes.  X = local x planes; lblk: across ranks the halo block holding the
// left x neighbour plane (-1: one rank, x periodic inside the slab).
struct Grid4 {
    int Ny = 0, Nvx = 0, Nvy = 0, X = 0;
    int lblk = -1;
    // across ranks, where the halo planes' columns sit in a row's stored (global column) order:
    // bit 0: the left plane's after the row (the slab starts at plane 0: its left is the last
    // plane), bit 1: the right plane's before it (the slab ends at the last plane)
    int xord = 0;
    const double *tab = nullptr;   // TX[2][Nvx] | TY[2][Nvy] | TVX[2][X] | TVY[2][Ny] (-, + each)
    const void *D = nullptr;       // diagonal per row, the operator's value type
};
inline size_t grid4_tab_len(const Grid4 &g) { return 2 * ((size_t)g.Nvx + g.Nvy + g.X + g.Ny); }
// k_g4_ring's limits (vtk_ring.hip): the LDS table TX | TY | TVX | TVY of <= G4TAB doubles and a
// ring of <= 8192 doubles holding the y-line window 2 S3 plus two groups of rows (512 per group for
// gr >= 512 outside the fused-dots mode 1, else 256).  The solver takes the ring step only for grids
// that fit (else the SELL grid-row kernels); launch_g4_ring refuses the others
constexpr int G4TAB = 1024;
constexpr int G4RM = 64;   // k_g4_ring: mirrored slots at each end of the x ring (> Nvy)
inline int g4_ring_group(int gr) { return gr >= 512 ? 512 : 256; }
// groups per workgroup of a k_g4_ring launch over ng groups of G rows for ~wgs workgroups,
// XCD-aligned: a workgroup's x -+ 1 plane rows belong to the workgroups q = S4 / (per G) indices
// away; per is rounded so that q is a multiple of 8, which puts them on the same XCD (workgroups
// are dealt round-robin over the eight XCDs) -- those reads hit its L2 (C4: per 48 -> 31, ring
// 384 -> 369 us)
// (only where a plane spans >= 8 groups and q would stay <= 32: with a few groups per
// workgroup the rounding cannot hold q near a multiple of 8)
inline int64_t g4_ring_per(int64_t ng, int64_t S4, int G, int wgs) {
    const int64_t per0 = std::max<int64_t>(1, (ng + std::max(1, wgs) - 1) / std::max(1, wgs));
    const double gpp = (double)S4 / G;   // groups per x-plane
    if (gpp < 8.0 || gpp / (double)per0 > 32.0) return per0;
    const int64_t q = std::max<int64_t>(8, (int64_t)std::ceil(gpp / (double)per0 / 8.0) * 8);
    return std::max<int64_t>(1, std::llround(gpp / (double)q));
}
inline bool g4_ring_fits(const Grid4 &g, int64_t n, int gr) {
    const int64_t S3 = (int64_t)g.Nvx * g.Nvy;
    return n > 0 && n <= INT32_MAX / 2 && 2 * S3 + 2 * g4_ring_group(gr) <= 8192 && grid4_tab_len(g) <= (size_t)G4TAB &&
           g.Nvy < G4RM;
}

// Tuning switches of a context (vtk_ctx_set_tuning): the defaults are the
// production path, the others exist for in-process A/B measurements and the bit-identity tests
// (the same sums with and without a byte-saving form).  Initialised from VTK_<KEY> (upper case)
// once, at vtk_ctx_create -- never read per launch.
struct Tuning {
    int band = 1;             // line-band DCGS2 step allowed (vtk_gmres_set_band)
    int band_lsv = 1;         // solver launches read the line-separable values (else SELL values)
    int sell_canon = 1;       // ... and canonical rows' columns from the line index (no codes)
    int band_canon = 1;       // the band step reads no codes on canonical rows
    int band_opt = 127;       // band step variant bits: every BandOpt bit (below, with each bit's measurements)
    int band_long_rows = 16000000;   // BAND_L2PF and BAND_ALT only on basis vectors of >= this many rows
                              // (in-process A/B, round 6: L2PF on vs off, C3 20M rows 39.30 vs 39.78 ms,
                              // C3/2 slab 10M 20.20 vs 20.09, C2 5M 10.98 vs 10.86, C3/8 slab 2.5M 6.53
                              // vs 6.51; ALT on vs off, C3 39.24 vs 39.34, C3/2 20.13 vs 20.00, C3/4
                              // 11.02 vs 10.95, C2 10.92 vs 10.87).  BAND_SERP does not follow it:
                              // faster at every size measured
    int lsv_ring = 2048;      // > 0: the line path's table SpMV with x staged through LDS, ~that many
                              // workgroups (in-process A/B, C3 line solve: 8.64 -> 8.26 ms; 167 -> 105 us)
    int prof_perj = 0;        // profile class per band step index (band_step_jNN)
    int comm_solo = 0;        // vtk_comm_init with world 1 builds a one-rank RCCL communicator
    int auto_band = 1;        // vtk_csr_create detects the line band and the 4D grid (drop-in path)
    int grid4 = 1;            // solver launches read 4D grid rows from their coordinates (Grid4)
    int c4_fused = 1;         // with grid4 and no ring: the DCGS2 dots fused into the 9-wide SELL step
    int g4_ring = 2048;       // > 0: the split step's SpMV + BJ of grid rows with x staged through LDS
                              // (k_g4_ring, ~that many workgroups), step 0's dots and the cycle-start
                              // residual in it too; takes precedence over c4_fused
    int g4_gr = 512;          // k_g4_ring: rows per group = lanes per workgroup (256 | 512)
    int g4_fast = 1;          // (A/B) k_g4_ring's straight-line sum for waves of inner rows
    int line_fuse = 1;        // line path (one rank, canonical rows): the SpMV inside the sweep kernel
    int line2_dc = 1;         // line product, DCGS2 step: the dots fused behind the second sweep
                              // (0: the plain second sweep, then launch_dc_dots; A/B and tests)
    int cyc_ring = 512;       // > 0: cycle-start residual and DCGS2 step 0 through the x-line ring
                              // (k_lsv_ring_epi, ~that many workgroups; 2D line-separable rows)
    int bcg_fuse = 1;         // BiCGStab with BJ, bs in {1, 2, 4, 8}: phat = M p and shat = M s inside
                              // k_bcg_p / k_bcg_s (0: the separate apply; the same bits either way)
    int linec_serial = 64;    // line_cyclic: a reduced level of at most this many unknowns per line is the
                              // last, solved by one lane per line (read at vtk_linecyclic_create)
    int neu_fuse = 1;         // Neumann wrapper around a BJ-fused base (bs <= 8): each correction
                              // w = z + M^-1 (r - A z) in one SpMV launch (0: residual SpMV, the base's
                              // apply, the addition -- the same bits; A/B and tests)
    int neu_dc = 1;           // Neumann wrapper, DCGS2 step: the step's dots behind the last correction's
                              // addition (0: the plain addition, then launch_dc_dots; A/B and tests)
    int fail_step = -1;       // (test hook) >= 0: this rank's DCGS2 step of that index fails in the
                              // first cycle as a refused launch would (the peer-failure vote, vtk_gmres);
                              // vtk_bicgstab: the first launch of that loop index is refused
};
}  // namespace vtk

struct vtk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;    // halo exchange overlapped with interior tiles
    hipEvent_t ev_pack = nullptr, ev_halo = nullptr;
    std::string err;
    int rank = 0, world = 1;
    bool dist = false;                    // distributed code paths: world > 1, or a one-rank
                                          // RCCL communicator (VTK_COMM_SOLO=1, testing)
    ncclComm_t comm = nullptr;            // RCCL (production transport)
    bool host_comm = false;               // host-staged hooks (vtk_comm_init_host)
    bool comm_broken = false;             // an RCCL call failed: vtk_ctx_destroy aborts the communicator
    vtk_host_comm hops{};
    int orth = VTK_ORTH_AUTO;
    int basis = VTK_BASIS_F64;            // vtk_gmres_set_basis: the Krylov basis' storage
    vtk_basis_info basis_info{};          // ... and what the last vtk_gmres used (vtk_gmres_basis_info)
    vtk::Tuning tune;                     // A/B switches (vtk_ctx_set_tuning), env at creation
    int n_cu = 0;                         // compute units (band step grid)
    // scratch shared by calls on this context
    double *d_part = nullptr;        // [8][GMAX] partial sums
    double *d_scal = nullptr;        // [256] reduced scalars (all-reduce slots)
    vtk::GmresState *d_state = nullptr;
    vtk::GmresState *h_state = nullptr;   // pinned mirror
    int *h_stop = nullptr;                // pinned, device-mapped: k_tail writes the stop column
    int *d_stop = nullptr;                // device alias of h_stop
    void *ws = nullptr;                   // solver workspace (grow-only, reused across solves)
    size_t ws_bytes = 0;
    // capture of one restart cycle (vtk_gmres_capture; a test hook, off by default)
    // cap: x_in[ld] | V[(m+1) ld] | H, S, giv | Hraw[(m+1)^2] | DcCoef
    int cap_cycle = -1;
    double *cap = nullptr;
    size_t cap_bytes = 0;
    bool cap_valid = false;
    vtk_arnoldi_info cap_info{};
    // kernel profile (vtk_profile_enable)
    struct ProfPending { int cls; int col; double bytes; hipEvent_t e0, e1; };
    struct ProfAcc { std::string name; int64_t launches = 0; double seconds = 0, bytes = 0; };
    bool prof_on = false;
    std::vector<ProfPending> prof_pending;
    std::vector<ProfAcc> prof_acc;
    std::vector<hipEvent_t> prof_pool;
};

struct vtk_csr {
    vtk_ctx *ctx = nullptr;
    int device = 0;   // the context's device: destroy never dereferences ctx (it may be gone)
    int64_t n_global = 0, row_begin = 0, row_end = 0, n_local = 0, nnz = 0;
    int fp32 = 0;
    int32_t *d_indptr = nullptr, *d_indices = nullptr;  // local column indices
    void *d_data = nullptr;
    std::vector<int32_t> h_indptr;                      // host copy (tile planning)
    std::vector<uint8_t> row_halo;                      // world > 1: row reads a halo column
    // SELL-64 layout (vtk_csr_set_layout): built when its padding is small (AUTO) or asked for
    vtk::Sell sell;
    bool use_sell = false;
    int layout = VTK_LAYOUT_AUTO;
    vtk::Groups g_all, g_in, g_bd;                      // g_in/g_bd: world > 1 (halo overlap)
    std::vector<int64_t> offsets;                       // partition, world+1
    vtk::Tiles tiles;                                   // align 1
    // halo (world > 1)
    int64_t n_halo = 0;
    std::vector<int64_t> halo_cols;                     // global ids, ascending
    std::vector<int64_t> recv_cnt, recv_off;            // per rank, into d_halo
    std::vector<int64_t> send_cnt, send_off;            // per rank, into d_send_buf
    double *d_halo = nullptr;
    int32_t *d_send_idx = nullptr;                      // local rows to pack
    double *d_send_buf = nullptr;
    int64_t n_send = 0;
    int64_t band_L = 0;                                 // line-band structure (vtk_csr_set_line_band)
    bool band_vloc = false;                             // ... with every column within v-1..v+1 of its row
    // line-separable values (k_lsv_build): every coupling to line x+-1 depends
    // only on the position v (table TX[2][L]), every coupling to v+-1 in the same line only on
    // the line x (TV[2][X]), the diagonal per row (D[n]) -- verified bit-exactly against the CSR
    // when the band is set; the band step then reads 8 B of values per row instead of 40.
    // d_lsv = D | TX | TV; null: not separable (the band step reads the SELL values)
    double *d_lsv = nullptr;
    bool lsv_canon = false;   // ... and every row canonical (canon_order): the band step reads no codes
    // 4D grid structure (vtk::Grid4; tables owned here); g4_dims = 0: not set
    vtk::Grid4 g4;
    double *d_g4tab = nullptr;
    void *d_g4D = nullptr;
    // distributed band step: the halo is two neighbour lines; peers and the alltoallv layout of
    // the per-step ghost exchange (BAND_GHOST_VECS L doubles per side), -1 offsets: no such side
    bool band_ghost = false;                            // band across ranks: per-step ghost exchange
    int band_lblk = 0;
    int band_xord = 0;                                  // bit 0: slab starts at global line 0, bit 1: ends at the last line
    int band_peer[2] = {-1, -1};                        // left, right neighbour rank
    std::vector<int64_t> band_scnt, band_soff, band_rcnt, band_roff;
    int64_t band_off_first = -1, band_off_last = -1;    // send offsets of the first / last line
    int64_t band_off_left = -1, band_off_right = -1;    // recv offsets of the left / right ghost
    // value updates (vtk_csr_update_values / vtk_csr_update_vlasov): the pattern and
    // everything planned from it stay, the values and the tables checked against them are redone
    int64_t values_epoch = 0;                           // successful updates since creation
    bool from_vlasov = false;                           // made by vtk_csr_create_vlasov ...
    vtk_vlasov_params vparams{};                        // ... from these parameters (the last update's)
    // the 4D grid geometry last tried on this operator (grid4_set; pointers null): an update
    // re-checks the new values against it, so tables lost to one set of values come back with the
    // next that passes.  Ny 0: none (never tried, or cleared by vtk_csr_set_grid4)
    vtk::Grid4 g4_try;
};

struct vtk_prec {
    vtk_csr *A = nullptr;
    int device = 0;   // destroy never dereferences A (a finaliser may have freed it first)
    int bs = 8;
    int64_t nb = 0;
    double *d_inv = nullptr;     // [nb][bs][bs]
    vtk::Tiles tiles;            // aligned to bs (fused SpMV + BJ)
    bool fused = false;          // fused SpMV+BJ kernel usable
    // world > 1, fused: the same tiles split into interior (no halo column: run while the halo
    // exchange is in flight) and boundary tiles (after it lands)
    vtk::Tiles tiles_in, tiles_bd;
    bool split = false;
    // tridiagonal blocks: LU factors l | m | g (SoA, stride tri_ld = nb * bs), vtk_bj_mode
    double *d_tri = nullptr;
    int64_t tri_ld = 0;
    bool tri_ok = false;
    int mode = VTK_BJ_AUTO;
    // line Jacobi (vtk_linejacobi_create): kind VTK_PREC_LINE, factors in line.f
    int kind = VTK_PREC_BJACOBI;
    vtk::LineOp line;
    bool line_compact_ok = false;   // x-invariant couplings found at setup (line.ac valid)
    // line product (vtk_lineproduct_create): kind VTK_PREC_LINE2, M = M1 D^-1 M2 with M1 = line,
    // M2 = line2 and d_diag = D, A's diagonal (n doubles)
    vtk::LineOp line2;
    bool line2_compact_ok = false;
    double *d_diag = nullptr;
    // periodic whole lines (vtk_linecyclic_create): kind VTK_PREC_LINEC
    vtk::LineC linec;
    // vtk_prec_refresh: what creation was asked for, and the operator values the
    // factors were computed from
    int setup = VTK_BJ_SETUP_EXACT;  // resolved vtk_bj_setup (EXACT or MFMA)
    int compact_req = -1;            // vtk_linejacobi_set_compact's last request (-1: none)
    int64_t epoch = 0;               // vtk_csr::values_epoch of the values M was factored from
    bool valid = true;               // false after a refresh that met a singular block / zero pivot
    // Neumann-series wrapper (vtk_neumann_create): kind VTK_PREC_NEUMANN.  The base
    // is borrowed, not owned: base_id is its serial in the registry of live preconditioners
    // (vtk_precond.cpp), checked before every use.  d_neu: three work vectors of n_local doubles
    uint64_t id = 0;                 // this preconditioner's serial in the registry (every kind)
    vtk_prec *base = nullptr;
    uint64_t base_id = 0;
    int degree = 1;
    double *d_neu = nullptr;
};

namespace vtk {

// ---- kernel launchers (vtk_kernels.hip) ------------------------------------------------------
struct SpmvIn {
    const int32_t *indptr, *indices;
    const void *data;
    int fp32;
    const Tiles *tiles;       // CSR-stream tiles (used when sell/groups are null)
    int n_local;
    const double *x, *halo;   // halo may be null (world == 1)
    const Sell *sell = nullptr;
    const Groups *groups = nullptr;
    // line-separable values (SELL, f64; solver launches only -- vtk_spmv keeps the SELL values)
    const double *lsv = nullptr;
    int lsv_L = 0, lsv_lblk = -1;
    int lsv_xord = 0;    // across ranks: the halo lines' place in the stored order (vtk_csr::band_xord)
    int lsv_canon = 0;   // ... and every row canonical: k_sell computes the columns (canon_row)
    int plain_grid = 0;  // workgroups of the plain SELL SpMV (0: 2 GMAX)
    Grid4 g4{};          // 4D grid rows (solver launches; g4.tab null: not used)
    int swz = 0;         // XCD-aware SELL group order: bit 0 the plain SpMV, bit 1 the other epilogues
    int plain_var = 0;   // plain SELL SpMV variant bits (k_sell VAR)
};

LineOp line_plan(int64_t n, int64_t row0, int64_t stride, int64_t seg);

// block-Jacobi operator as the kernels see it: inverse rows f64[nb][bs][bs], or (tri != null)
// the LU factors of tridiagonal blocks, SoA l | m | g with stride tri_ld (vtk_driver.hpp bj_op, BJ
// modes).  bs == 0: identity.  The other kinds have no such form: vtk_apply.cpp launches them
struct BjOp {
    const double *inv = nullptr;
    const double *tri = nullptr;
    int64_t tri_ld = 0;
    int bs = 0;
};

// mm[0] = min, mm[1] = max of idx[0..n) (mm preset to INT_MAX, INT_MIN)
hipError_t launch_index_range(const int32_t *idx, int64_t n, int *mm, hipStream_t s);

// workgroups (= partials) of a launch on this input
inline int spmv_grid(const SpmvIn &in) { return (in.sell && in.groups) ? in.groups->grid : in.tiles->grid; }

// EPI_PREC_DC: w = M^-1 A p_j plus the DCGS2 step's dot products (launch_spmv_dc)
// EPI_PREC_DC_ND (launch_lsv_ring_epi only): EPI_PREC_DC as w = p_j + M^-1 (A - M) p_j, D not read
// EPI_NEU_RESID: y = b - A x and nothing else (the Neumann wrapper's residual)
// EPI_NEU_CORR: y = x + M^-1 (b - A x), one correction of the wrapper in one launch (BJ-fused tiles,
// bs <= 8; tridiagonal blocks solved with the stored l | m | g, as launch_bj_apply does)
enum Epi { EPI_PLAIN = 0, EPI_RESID = 1, EPI_PREC = 2, EPI_RESID_PREC = 3, EPI_PREC_DC = 4, EPI_PREC_DC_ND = 5,
           EPI_NEU_RESID = 6, EPI_NEU_CORR = 7 };

// y = A x (PLAIN); y = b - A x, part0 = sum y^2 (RESID); y = M^-1 A x with M = BJ(inv, bs)
// or identity (inv == null), part0 = sum y^2, part1 = sum v0*y (PREC, v0 may be null);
// RESID_PREC: r = b - A x, y = M^-1 r, part0 = sum r^2, part1 = sum y^2.
// NEU_RESID: y = b - A x, no partials.  NEU_CORR: y = x + M^-1 (b - A x) (y must not alias x);
// part0 = sum y^2 and part1 = sum v0*y when part0 is given (the wrapper's last correction).
hipError_t launch_spmv(const SpmvIn &in, int epi, double *y, const double *b, const BjOp &bj,
                       const double *v0, double *part0, double *part1,
                       const int *stop_col, int col, hipStream_t s);
// z = M^-1 r (BJ or identity when inv == null); part0 = sum z^2, part1 = sum v0*z (optional)
hipError_t launch_bj_apply(const BjOp &bj, int64_t n, const double *r, double *z,
                           const double *v0, double *part0, double *part1, int grid,
                           const int *stop_col, int col, hipStream_t s);
// factors of tridiagonal diagonal blocks (bs in {2, 4, 8}): tri[i] = l_i, tri[ld + i] = m_i = 1/u_i,
// tri[2 ld + i] = g_i = sup_i m_i (Thomas, no pivoting); *flags |= 1 a block is not tridiagonal,
// 2 a pivot is tiny, 4 the factors disagree with the Gauss-Jordan inverse beyond 1e-10
// SELL-64 build: phase 0 = chunk widths + scan into off (scan_tmp of sell_scan_bytes(n),
// tmp64 of nch+1 int64), phase 1 = fill col/val
hipError_t launch_sell_build(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                             int64_t *off, int64_t *tmp64, void *scan_tmp, size_t scan_bytes, int32_t *col,
                             void *val, int phase, hipStream_t s);
size_t sell_scan_bytes(int64_t n);
// dictionary-coded columns of a built SELL: phase 0 = word offsets + scan into pkoff (tmp64
// [nch+1], scan_tmp as above), phase 1 = codes + dictionaries, n_wide counted into *wide_cnt
hipError_t launch_sell_pack(const int64_t *off, int64_t nch, int64_t *pkoff, int64_t *tmp64, void *scan_tmp,
                            size_t scan_bytes, const int32_t *col, uint32_t *pk, int32_t *dict,
                            unsigned long long *wide_cnt, int phase, hipStream_t s);
// line Jacobi: factors (flags: *bad_row = min global row with a zero / non-finite pivot; ext:
// 4 jn words, per line min/max bit patterns of the a's and c's, init ~0 / 0 / ~0 / 0) and
// z = M^-1 r with part0 = sum z^2, part1 = sum v0*z (optional) over `grid` workgroups
hipError_t launch_line_setup(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                             const LineOp &L, unsigned long long *bad_row, unsigned long long *ext, hipStream_t s);
// z = M_line^-1 r fused with DCGS2 step j's dots (p = the SpMV input, partials in the
// launch_dc_dots layout); hipErrorInvalidValue when the segments are too long (> 32)
// zadd (here and in the sweeps below; the Neumann wrapper's correction): the last
// write stores zadd + M^-1 r instead, and the partials / dots are those of the stored sum; the
// output must not alias zadd
hipError_t launch_line_dc(const LineOp &L, const double *r, double *w, const double *V, int64_t ld, int j,
                          const double *p, double *part, int grid, const int *stop_col, int col, hipStream_t s,
                          const double *zadd = nullptr);
// the same with y = A p formed inside (k_line_spmv_dc): one rank, canonical line-separable rows
// (lsv: vtk_csr::d_lsv), lines of L.stride rows, compact factors; hipErrorInvalidValue otherwise
hipError_t launch_line_spmv_dc(const LineOp &L, const double *lsv, const double *p, double *w, const double *V,
                               int64_t ld, int j, double *part, int grid, const int *stop_col, int col, hipStream_t s);
hipError_t launch_line_apply(const LineOp &L, const double *r, double *z, const double *v0, double *part0,
                             double *part1, int grid, const int *stop_col, int col, hipStream_t s,
                             const double *zadd = nullptr);
// line product, second sweep (vtk_line2.hip): z = M_L^-1 (D t), the forward sweep's right-hand side
// formed as D[k] t[k] per row; t and z may alias.  Partials as launch_line_apply / launch_line_dc
// (the DCD form: segments <= 32, else hipErrorInvalidValue).  launch_line2_diag: D[r] = the sum of
// row r's stored entries with col == row, in stored order from 0.0 (k_line_setup's b)
hipError_t launch_line2_diag(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                             double *D, hipStream_t s);
hipError_t launch_line2_apply(const LineOp &L, const double *D, const double *t, double *z, const double *v0,
                              double *part0, double *part1, int grid, const int *stop_col, int col, hipStream_t s,
                              const double *zadd = nullptr);
hipError_t launch_line2_dc(const LineOp &L, const double *D, const double *t, double *w, const double *V, int64_t ld,
                           int j, const double *p, double *part, int grid, const int *stop_col, int col, hipStream_t s,
                           const double *zadd = nullptr);
// periodic whole lines (vtk_linec.hip).  launch_linec_setup: level lev's factors and spikes (level
// 0 from the CSR, else from co = a | b | c), then its separators' system into co (the next level's
// coefficients) or, at the last level, C.minv; bad[lev] / bad[nlev]: the smallest element index of
// that level / of the last level's pivots that is zero or not finite (preset ~0).
// launch_linec_phase: 0 the level-0 sweep (y into z's interior rows), 1 the separators' right-hand
// sides and every reduced level, 2 the level-0 correction with part0 = sum z^2, part1 = sum v0 z
// over grid workgroups.  r and z may alias
hipError_t launch_linec_setup(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                              const LineC &C, int lev, double *co, unsigned long long *bad, hipStream_t s);
hipError_t launch_linec_phase(const LineC &C, int phase, const double *r, double *z, const double *v0, double *part0,
                              double *part1, int grid, const int *stop_col, int col, hipStream_t s,
                              const double *zadd = nullptr);   // (zadd: phase 2 only)
// the rank level of lines that span the ranks (C.sp).  _rhs: rhs = 0 but a_first in
// the first local rows (which 0) or c_last in the last (which 1), each the row's stored entries at
// the column C.sp.ecol names, summed in stored order from 0.0.  _tips: C.sp.tsend from C.sp.vw.
// _edge: C.sp.edge from the sweep's y in z and level 1's solution (after phases 0 and 1).  _iface:
// C.sp.xe from C.sp.tips and C.sp.edges, every rank's interface system solved per line (no
// pivoting); bad (setup; optional): the smallest j whose system has a zero or non-finite pivot.
// _correct: phase 2 with the rank terms fused in, partials as launch_linec_phase's
hipError_t launch_linec_span_rhs(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                                 const LineC &C, int which, double *rhs, hipStream_t s);
hipError_t launch_linec_span_tips(const LineC &C, hipStream_t s);
hipError_t launch_linec_span_edge(const LineC &C, const double *z, const int *stop_col, int col, hipStream_t s);
hipError_t launch_linec_span_iface(const LineC &C, unsigned long long *bad, const int *stop_col, int col, hipStream_t s);
hipError_t launch_linec_span_correct(const LineC &C, double *z, const double *v0, double *part0, double *part1,
                                     int grid, const int *stop_col, int col, hipStream_t s);
// Neumann wrapper (vtk_neumann.hip): w = z + u, one addition per row, with
// part0 = sum w^2 and part1 = sum v0 w (optional) over `grid` workgroups; w may alias z or u.
// launch_neu_add_dc: the same addition with DCGS2 step j's dots behind it (p = V[j], the partials in
// launch_dc_dots' layout), so that no dots kernel re-reads w
hipError_t launch_neu_add(const double *z, const double *u, double *w, int64_t n, const double *v0, double *part0,
                          double *part1, int grid, const int *stop_col, int col, hipStream_t s);
hipError_t launch_neu_add_dc(const double *z, const double *u, double *w, int64_t n, const double *V, int64_t ld,
                             int j, double *part, int grid, const int *stop_col, int col, hipStream_t s);
hipError_t launch_bj_tri_setup(const int32_t *indptr, const int32_t *indices, const void *data, int fp32,
                               int64_t n, int bs, const double *inv, double *tri, int64_t ld, int *flags,
                               hipStream_t s);
hipError_t launch_bj_setup(const int32_t *indptr, const int32_t *indices, const void *data,
                           int fp32, int64_t n, int bs, double *inv, int *d_singular,
                           double *work, hipStream_t s);
// the same inverses for bs 16 / 32 by blocked Gauss-Jordan on the matrix cores (k_bj_setup_mfma;
// agrees with launch_bj_setup to rounding, not bit for bit)
hipError_t launch_bj_setup_mfma(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                                int bs, double *inv, int *d_singular, hipStream_t s);
// w -= h v_k with h = reduce(hin); part_out = sum v_next*w (or sum w^2 if v_next == null)
hipError_t launch_mgs(Red hin, double *hout, double *w, const double *vk, const double *vnext,
                      int64_t n, double *part_out, int grid, const int *stop_col, int col,
                      hipStream_t s);
// h0 = sqrt(reduce(h0)), h1 = sqrt(reduce(w2)); v_next = w * (1/h1) (w if breakdown);
// workgroup 0 applies the Givens rotations to column col of H and sets the stop flag.
hipError_t launch_tail(Red h0, Red w2, const double *w, double *vnext, int64_t n, int col,
                       int m, double *H, double *S, double *giv, GmresState *st, int *stop_map,
                       int grid, hipStream_t s);
// v0 = v0 * (1/t), t = sqrt(reduce(p)); S[0] = t, S[1..m] = 0, stop_col = BIG_COL
hipError_t launch_scale0(Red p, double *v0, int64_t n, double *S, int m, GmresState *st,
                         int grid, hipStream_t s);
// y = triangular solve (H, S) at stop column; x += y @ V
// (returns at entry when a DCGS2 update pass already did it: st->xup_tag >= 0)
hipError_t launch_xupdate(const double *H, const double *S, const double *V, int64_t ld,
                          double *x, int64_t n, int m, const GmresState *st, int grid, hipStream_t s);
// dst = sqrt(reduce(p)) if do_sqrt else reduce(p)   (single workgroup)
hipError_t launch_finalize(Red p, double *dst, int do_sqrt, hipStream_t s);
// part = sum x^2 (or x*y)
hipError_t launch_dot(const double *x, const double *y, int64_t n, double *part, int grid,
                      hipStream_t s);
// *flag = 1.0 when some x[i] != 0 (zeroed by the caller)
hipError_t launch_any_nonzero(const double *x, int64_t n, double *flag, hipStream_t s);
hipError_t launch_gather(const double *x, const int32_t *idx, int64_t cnt, double *out,
                         hipStream_t s);
// device operator assembly
hipError_t launch_vlasov_counts(const vtk_vlasov_params &p, int64_t r0, int64_t nrows,
                                int32_t *counts, hipStream_t s);
hipError_t launch_vlasov_fill(const vtk_vlasov_params &p, int64_t r0, int64_t nrows,
                              const int32_t *indptr, int32_t *indices, void *data,
                              hipStream_t s);
// value updates (vtk_update.hip): the SELL copy's values from the CSR values, the pattern (off,
// columns, codes) untouched -- k_sell_fill's values bit for bit; and the Vlasov generator's values
// of rows [r0, r0 + nrows) into data at the existing indptr, no column written
hipError_t launch_sell_refresh(const int32_t *indptr, const void *data, int fp32, int64_t n, const int64_t *off,
                               void *val, hipStream_t s);
hipError_t launch_vlasov_values(const vtk_vlasov_params &p, int64_t r0, int64_t nrows, const int32_t *indptr,
                                void *data, hipStream_t s);
hipError_t launch_exclusive_scan(const int32_t *in, int32_t *out, int64_t n, void *tmp,
                                 size_t *tmp_bytes, hipStream_t s);
hipError_t launch_remap_cols(int32_t *indices, int64_t nnz, int64_t row_begin, int64_t n_local,
                             const int64_t *halo_cols, int64_t n_halo, hipStream_t s);

// DCGS2: dots pass (s = V_j^T p_j, z = V_j^T w, alpha, beta, gamma; w == null: s, alpha only),
// per-quantity finalize (one workgroup per quantity), single-lane scalar step, update pass.
hipError_t launch_dc_dots(const double *V, int64_t ld, int j, const double *w, int64_t n,
                          double *part, int grid, const int *stop_col, int col, hipStream_t s);
// DCGS2 step j fused into the SpMV: w = M^-1 A p_j with p_j = V[j] (in.x), and per workgroup
// the partials of s = V_j^T p_j, z = V_j^T w, |p|^2, p.w, |w|^2 (layout of launch_dc_dots);
// grid = tiles->grid partials.  BJ-fused tiles with bs in {1, 2, 4, 8} only.
hipError_t launch_spmv_dc(const SpmvIn &in, double *w, const BjOp &bj, const double *V,
                          int64_t ld, int j, double *part, const int *stop_col, int col, hipStream_t s);
hipError_t launch_dc_finalize(const double *part, int cnt, int j, int with_w, double *scal,
                              const int *stop_col, int col, hipStream_t s);
// part != null: reduce the G partials in-kernel (one GPU); else read the all-reduced scal
// r_meas: step 0 measures ||v_0|| = sqrt(alpha) instead of taking 1 (the compressed basis)
hipError_t launch_dc_scalar(const double *part, int cnt, const double *scal, int j, int m,
                            int closing, double *Hraw, double *H, double *S, double *giv,
                            DcCoef *cf, GmresState *st, int *stop_map, hipStream_t s, int r_meas = 0);
// update pass of step j; when the step's scalar kernel stopped the cycle (st->xup_tag == j) it
// does the cycle's x update instead: x += V[0..c] y, y = H^-1 S at c = stop_col (j-1 or j; for
// c = j the v_j of the pass is formed in registers), reading the basis once
hipError_t launch_dc_update(double *V, int64_t ld, int j, const double *w, int64_t n,
                            const DcCoef *cf, int grid, const GmresState *st, double *x,
                            const double *H, const double *S, int m, int nt_pw, hipStream_t s);

// Compressed basis (vtk_gmres_set_basis VTK_BASIS_F32; vtk_cbasis.hip): the split DCGS2
// step's passes with the finalised columns in Vc[(m + 1) x ld] floats and the candidates p_j, p_{j+1} in
// two float64 vectors.  Partials, stop test, coefficients and the x update's rule as the float64
// launches above; every pointer 16-byte aligned, ld a multiple of 4 (hipErrorInvalidValue otherwise).
// launch_cb_scale0: p0 = p0 / sqrt(reduce(p)), Vc[0] = (float) p0, p0 = (double) Vc[0]
hipError_t launch_cb_scale0(Red p, double *p0, float *Vc, int64_t n, double *S, int m, GmresState *st, int grid,
                            hipStream_t s);
hipError_t launch_cb_dots(const float *Vc, int64_t ld, int j, const double *p, const double *w, int64_t n,
                          double *part, int grid, const int *stop_col, int col, hipStream_t s);
// reads p_j (pj) and w, stores Vc[j] (j >= 1) and p_{j+1} (pn != pj); st->xup_tag == j: the x update
hipError_t launch_cb_update(float *Vc, int64_t ld, int j, const double *pj, const double *w, double *pn, int64_t n,
                            const DcCoef *cf, int grid, const GmresState *st, double *x, const double *H,
                            const double *S, int m, hipStream_t s);
hipError_t launch_cb_xupdate(const double *H, const double *S, const float *Vc, int64_t ld, double *x, int64_t n,
                             int m, const GmresState *st, int grid, hipStream_t s);
// the capture hook's V: the m + 1 columns widened, the open candidate (pa / pb by parity) in its column
hipError_t launch_cb_capture(const float *Vc, int64_t ld, int m, const double *pa, const double *pb,
                             const GmresState *st, double *out, hipStream_t s);

// Variant bits of the band step (Tuning::band_opt -> StepPlan::band_opt -> BandK::opt), for the
// canonical-row kernels (VMODE 2) only: step_plan masks them off elsewhere.  Compile-time bits pick
// the instantiation (k_band_step's OPT, through vtk_band.hip band_variant); run-time bits are read
// from a.opt inside the kernel.  All variants compute the same w and partial sums, except: WPC3's
// grid (more, shorter line ranges), ALT and SERP (a reversed walk sums a range's lines in reverse
// order) change the dots' summation order, ND the last bits of w -- all within the DCGS2 bars.
enum BandOpt : int {
    // compile-time.  With the next-line prefetch (J <= BAND_PF), the SpMV operands of a line (D, m,
    // the line's v couplings) travel in the same prefetch as the update operands, one line ahead.
    // Loaded at the head of their own iteration they made the wait for the prefetched update
    // operands a wait for everything (s_waitcnt vmcnt(0): the loads sit in exec-masked blocks, so
    // the counter cannot be tracked per load): one exposed memory round trip per line.  (C3: j00 254
    // -> 217 us.)  Launched only at the step indices where it pays (vtk_band.hip band_spf_j)
    BAND_SPF = 1,
    // compile-time, and the host's grid (Solver::band_grid).  Registers capped for 3 workgroups per
    // CU (6 waves per SIMD) at J <= BAND_J3 (below), whose serial line walks are latency-bound; the
    // host plans 1.5x the line ranges for them.  (C3, on top of SPF: j00 190, j01 283 -> 246 us;
    // solve 42.66 -> 42.31 ms)
    BAND_WPC3 = 2,
    // run-time.  The two parts of a line range on ONE XCD.  Each part updates one v-halo row on
    // either side, which lies in the other part's rows: read alone, that row drags its whole 128-B
    // line from HBM (the band step's PMC fetch is ~9 % over its algorithmic bytes at j >= 9).
    // Workgroups are dealt to the XCDs round-robin (blockIdx mod 8): vtk_band.hip band_block remaps
    // them.  (Round 6: 40.56 -> 40.30 ms)
    BAND_XCDP = 4,
    // compile-time, J > BAND_PF only (step_plan: long basis vectors only, Tuning::band_long_rows).
    // The global rows a later line iteration reads -- its update's basis and w rows, its SpMV's D
    // and m rows -- are touched ahead of time by LDS-DMA loads into a scratch word nobody reads: no
    // VGPR holds them, so the walk keeps more bytes in flight than the register prefetch alone (one
    // line ahead without it, J > BAND_PF; two with it).  The barriers then are bare s_barriers
    // (vtk_band.hip band_sync).  (j13-j18 -21..-50 us each)
    BAND_L2PF = 8,
    // run-time (long basis vectors only, as L2PF).  Odd line ranges walk their lines backwards, so
    // that the two workgroups on either side of every range boundary read the boundary's two lines
    // (each one's own line and the other's x-halo line) at the same time, at the start or at the
    // end of both walks: the second read finds the line in the Infinity Cache instead of HBM.
    // (39.98 -> 39.81 ms, C3/8 slab 6.652 vs 6.676 ms (neutral).  Since round 6 also across ranks)
    BAND_ALT = 16,
    // run-time (against the template's J: no cost).  Odd steps walk the other way round, on top of
    // ALT's range parity, so step j + 1 begins with the lines step j touched last -- the rows it
    // reads there (V_k, v_j, both w, D, m) were read or written a few hundred MB of traffic earlier
    // and are still in the Infinity Cache.  The non-temporal loads and write-through
    // stores leave their lines there as plain ones do (profiles/serpentine_probe.txt), so the load
    // and store policies are the same at both ends of a walk as in its middle.  (C3 37.37 -> 36.62
    // ms (two runs: -2.0 %, -1.7 %), at every size: C2 10.28 -> 10.21, C3/2 slab 18.95 -> 18.86,
    // C3/8 slab 6.23 -> 6.16 ms (profiles/serpentine_ab*.json); every step reversed instead of
    // every other one: 38.79 vs 38.78 ms, nothing)
    BAND_SERP = 32,
    // compile-time; also step 0 of the band's cycle (EPI_PREC_DC_ND).  No read of the diagonal table
    // D.  The band step runs only with the tridiagonal BJ(8) factors of A's current diagonal blocks
    // (bj_op() hands out tri for the operator's current values_epoch only; the launch site in
    // vtk_gmres.cpp states the guard), so A = M + C with C the x +- 1 couplings and the v +- 1
    // couplings that cross an 8-row block edge, and
    //   w = M^-1 A p = p + M^-1 (C p):
    // the row sum y = C p skips the diagonal and the in-block v +- 1 products (the in-block
    // couplings still enter bj_trim_group as sub / sup, from the per-line constants), z = M^-1 y,
    // w = p + z.  One 8-B stream per row fewer (load, SPF operand, L2PF row); w differs from the D
    // form in its last bits only
    BAND_ND = 64,
};

// Line-band DCGS2 step (k_band_step): update pass of step j + SpMV, tridiagonal
// BJ(8) and dots of step j+1 in one sweep over x-lines of L rows (SELL-64 uniform width 5, coded
// columns, fp64 values; across ranks through the ghost lines).  grid workgroups (<= X lines, <= GMAX), partials of step j+1 in
// the launch_dc_dots layout.  p_j is recomputed from w_{j-1} (w_prev) and stored only for
// j + 1 = m - 1 (k_dc_update's operand); w rotates over three buffers.
struct BandK {
    const uint32_t *pk;
    const int32_t *dict;
    const double *val;
    const double *mtri;
    double *V;
    int64_t ld;
    int j, m;
    const double *w_in;          // w_j
    const double *w_prev;        // w_{j-1} (unused at j = 0)
    double *w_out;               // w_{j+1}
    const DcCoef *cf;
    const GmresState *st;
    double *x;
    const double *H, *S;
    double *part;
    int64_t n;
    int L, X, H_parts;           // line length, lines, parts per line (grid = ranges x H_parts)
    const double *ghost;         // distributed: [2][m+2][L] the left / right neighbour lines'
                                 // v_k (k < j) and w_j, w_{j-1} by parity in slots m, m+1
                                 // (k_ghost_unpack); null on one rank
    int left_blk;                // halo block (0 / 1) holding the left neighbour line
    int xord = 0;                // bit 0: the slab starts at global line 0, bit 1: ends at the last line
    const double *lsv;           // line-separable values (vtk_csr::d_lsv) or null: SELL values
    bool canon;                  // with lsv: canonical rows (vtk_csr::lsv_canon), no codes read (VMODE 2)
    int opt = 0;                 // BandOpt bits
};
hipError_t launch_band_step(const BandK &a, int grid, int wu, hipStream_t s);
// geometry (k_band_step): a workgroup of BAND_T threads owns <= BAND_LP rows of a
// line (one part; parts per line = band_parts), BAND_WPC workgroups per CU (LDS-bound)
constexpr int BAND_LP = 400, BAND_T = 448, BAND_WPC = 2;
constexpr int BAND_JV = 19;    // basis vectors staged per line (j + 1 <= 19: restart <= 20)
// band steps j <= BAND_J3 run three workgroups per CU (BAND_WPC3): their LDS (ring +
// (j + 1) staged basis rows of BAND_LP doubles) fits three times into 160 KB, and their registers
// the 80-VGPR cap (j = 3 / 4 fit too since the x update is inline, but measured within noise)
constexpr int BAND_J3 = 2;
// vectors per ghost line and step of the distributed band step: v_{j-1} (v_0 at j = 0), w_j
constexpr int BAND_GHOST_VECS = 2;
hipError_t launch_band_check_dist(const int32_t *indptr, const int32_t *indices, int64_t n, int L, int lblk, int *bad,
                                  hipStream_t s);
hipError_t launch_ghost_pack(const double *V, int64_t ld, int j, const double *w, int64_t n, int L, double *sbuf,
                             int64_t off_first, int64_t off_last, hipStream_t s);
hipError_t launch_ghost_unpack(const double *rbuf, int64_t off_left, int64_t off_right, int j, int m, int L,
                               double *ghost, hipStream_t s);
int band_parts(int64_t L, int lp = BAND_LP);   // parts per line (rows per part <= lp, multiple of 8); 0: none (vtk_host.cpp)
// *bad |= 1 when some column is outside the lines x-1..x+1 (mod X) of its row, |= 2 when one is
// more than one row off its row's position in the line (bad zeroed by the caller)
// line-separable values (vtk_csr::d_lsv): build D | TX | TV from the CSR, then *bad |= 1 when
// some entry is not reproduced bit-exactly (or is no diagonal / v+-1 / same-position x+-1
// coupling).  lblk < 0: one rank (x couplings periodic); else the halo block of the left line
hipError_t launch_lsv_build(const int32_t *indptr, const int32_t *indices, const double *data, int64_t n, int L,
                            int lblk, int xord, double *lsv, int *bad, hipStream_t s);
// y = A x from the line-separable tables and the SELL codes (uniform width 5, coded columns):
// k_sell's plain SpMV, the same bits.  halo != null: the distributed layout (lblk the left block)
// the x-line ring SpMV with the solver's epilogues (one rank, canonical rows; k_lsv_ring_epi):
// EPI_RESID (y = b - A x, p0 = |r|^2 partials), EPI_RESID_PREC (y = M^-1 (b - A x), p0, p1 =
// |r|^2, |z|^2), EPI_PREC_DC (y = M^-1 A x, DCGS2 step-0 dots |x|^2, x.y, |y|^2 into dcpart;
// EPI_PREC_DC_ND: the same without the read of D);
// *grid_out partials (<= GMAX)
hipError_t launch_lsv_ring_epi(int epi, const double *lsv, const double *x, const double *b, const double *mtri,
                               double *y, double *p0, double *p1, double *dcpart, int64_t n, int L, int ring_wgs,
                               const int *stop_col, int col, int *grid_out, hipStream_t s, const double *halo = nullptr,
                               int lblk = -1, int xord = 0);   // halo: across ranks, the two neighbour lines
hipError_t launch_lsv_spmv(const uint32_t *pk, const int32_t *dict, const double *lsv, const double *x,
                           const double *halo, double *y, int64_t n, int L, int lblk, const int *stop_col, int col,
                           hipStream_t s, int canon, int grid_cap,
                           int ring_wgs = 0, int xord = 0);   // canon: rows canonical, no codes read; ring_wgs > 0: LDS-staged x
                                                // (k_lsv_ring, about that many workgroups; one rank, canon)
// 4D grid tables (vtk::Grid4) from the CSR (pass 0) and the check (pass 1): *bad |= 1 when an entry
// is no grid coupling or differs from its table value, |= 2 when a row is not in ascending
// canonical order; D and tab written here
hipError_t launch_grid4_build(const int32_t *indptr, const int32_t *indices, const void *data, int fp32, int64_t n,
                              const Grid4 &g, double *tab, void *D, int *bad, hipStream_t s);
// w = M^-1 A x for 4D grid rows with x staged through LDS (k_g4_ring): the tridiagonal BJ(8) of
// m = mtri; about wgs workgroups, each a contiguous range of 256-row groups; halo != null: across
// ranks (g.lblk the left plane's halo block).  Bit-identical to the SELL launch.  dots != null:
// DCGS2 step 0's dots (mode 2: |p|^2, p.w, |w|^2) or the cycle-start residual (mode 3, w = M^-1
// (b - A x)); partials per workgroup (at most GMAX workgroups, the count in *grid_out).
struct G4Dots {
    int mode = 2;                  // 2: step 0's dots; 3: cycle-start residual
    double *part = nullptr;        // mode 2: the dots partials (launch_dc_dots' layout)
    const double *b = nullptr;     // mode 3: the right-hand side; |r|^2, |w|^2 partials
    double *p0 = nullptr, *p1 = nullptr;
    int part_off = 0;              // the launch's first partial slot (split launches side by side)
};
// g_lo, g_hi: the group range (GR-row groups; -1: all), per: groups per workgroup (0: from wgs)
hipError_t launch_g4_ring(const Grid4 &g, const double *x, const double *halo, const double *mtri, double *w, int64_t n,
                          int fp32, int wgs, int gr, const G4Dots *dots, int *grid_out, const int *stop_col,
                          int col, hipStream_t s, int g_lo = 0, int g_hi = -1, int per = 0, int fast = 1);
hipError_t launch_band_check(const int32_t *indptr, const int32_t *indices, int64_t n, int L, int X, int *bad,
                             hipStream_t s);

int vector_grid(int64_t n);

// ---- BiCGStab (vtk_bicgstab.hip) -------------------------------------------------------------
// every launch: grid workgroups of NT threads (vector_grid), returns at entry once *stop < tag
// bj usable by the fused forms: block Jacobi, bs in {1, 2, 4, 8} (tridiagonal factors: 2, 4, 8)
bool bcg_fusable(const BjOp &bj);
// p = r + beta (p - omega v) with beta, omega from st (first: p = r); bj != null: also phat = M^-1 p
hipError_t launch_bcg_p(const BicgState *st, int first, int64_t n, const double *r, const double *v, double *p,
                        const BjOp *bj, double *phat, int grid, const int *stop, int tag, hipStream_t s);
// s = r - alpha v in place, part = sum s^2; bj != null: also shat = M^-1 s
hipError_t launch_bcg_s(const BicgState *st, int64_t n, double *r, const double *v, const BjOp *bj, double *shat,
                        double *part, int grid, const int *stop, int tag, hipStream_t s);
// omega = reduce(ts) / reduce(tt); x += alpha phat + omega shat; r = s - omega t (in place);
// part_rr = sum r^2, part_rho = sum rtilde r.  vote != null (across ranks): the vote slot of the
// omega record; nonzero: the kernel returns with x and r untouched
hipError_t launch_bcg_x(const BicgState *st, Red ts, Red tt, int64_t n, double *x, const double *phat,
                        const double *shat, double *r, const double *t, const double *rtilde, double *part_rr,
                        double *part_rho, const double *vote, int grid, const int *stop, int tag, hipStream_t s);
// x += alpha phat, only when *stop == tag (the half-step exit of that iteration fired)
hipError_t launch_bcg_half_x(const BicgState *st, int64_t n, double *x, const double *phat, int grid, const int *stop,
                             int tag, hipStream_t s);
// the scalar step (one workgroup), phase BCG_PH_*; unused quantities: Red{nullptr, 0}.  vote != null
// (across ranks): the vote slot of the record the quantities come from; nonzero: BicgState::peer_failed
// and a stop at this step
hipError_t launch_bcg_scalar(int phase, int64_t k, int last, int info_max, double atol, Red q0, Red q1, Red q2, Red q3,
                             const double *vote, BicgState *st, int *stop_map, const int *stop, int tag,
                             hipStream_t s);
// across ranks (one workgroup): rec[i] = reduce(q_i) for i < nq <= 4, rec[nq] = *my_vote; the driver
// all-reduces rec[0..nq]
hipError_t launch_bcg_reduce(Red q0, Red q1, Red q2, Red q3, int nq, const double *my_vote, double *rec,
                             const int *stop, int tag, hipStream_t s);

// ---- host helpers (vtk_host.cpp) -------------------------------------------------------------
void build_tiles(const std::vector<int32_t> &indptr, int align, std::vector<int32_t> &rows,
                 bool &has_long, bool &aligned);
void set_context_free_error(const std::string &msg);

}  // namespace vtk
