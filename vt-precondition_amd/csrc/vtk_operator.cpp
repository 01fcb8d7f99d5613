// vtk_operator.cpp -- layout and setup of a vtk_csr: tiles, the SELL-64 copy and its coded columns,
// groups, the halo plan, line-band and 4D-grid detection, value updates.
#include <climits>
#include <cstdlib>

#include "vtk_driver.hpp"

using namespace vtk;

namespace vtk {

int upload_tiles(vtk_ctx *c, const std::vector<int32_t> &indptr, int align, Tiles &t,
                 std::vector<int32_t> *rows_out) {
    std::vector<int32_t> rows;
    build_tiles(indptr, align, rows, t.has_long, t.aligned);
    if (rows_out) *rows_out = rows;
    t.ntiles = (int)rows.size() - 1;
    t.align = align;
    t.grid = grid_for(c, std::max(1, std::min(t.ntiles, GMAX)));
    if (t.d_row) (void)hipFree(t.d_row);
    t.d_row = nullptr;
    HIPCHK(c, hipMalloc(&t.d_row, rows.size() * sizeof(int32_t)));
    HIPCHK(c, hipMemcpy(t.d_row, rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return VTK_OK;
}

void free_tiles(Tiles &t) {
    (void)hipFree(t.d_row);
    (void)hipFree(t.d_end);
    t.d_row = t.d_end = nullptr;
}

// Split the tiles of `all` (host row boundaries `rows`) into interior tiles (no row reads a halo
// column) and boundary tiles, as [start, end) lists.  Grids: boundary <= 64 workgroups,
// interior the rest of GMAX, so both launches' partials fit one GMAX-strided slot row.
int upload_split_tiles(vtk_ctx *c, const std::vector<int32_t> &rows, const std::vector<uint8_t> &row_halo,
                       const Tiles &all, Tiles &in, Tiles &bd) {
    std::vector<int32_t> is, ie, bs_, be;
    for (size_t t = 0; t + 1 < rows.size(); ++t) {
        bool h = false;
        for (int32_t r = rows[t]; r < rows[t + 1] && !h; ++r) h = row_halo[(size_t)r] != 0;
        (h ? bs_ : is).push_back(rows[t]);
        (h ? be : ie).push_back(rows[t + 1]);
    }
    auto up = [&](const std::vector<int32_t> &st, const std::vector<int32_t> &en, Tiles &t, int gmax) -> int {
        free_tiles(t);
        t.ntiles = (int)st.size();
        t.align = all.align;
        t.has_long = all.has_long;
        t.aligned = all.aligned;
        t.grid = std::max(1, std::min(t.ntiles, gmax));
        t.nrows = 0;
        for (size_t k = 0; k < st.size(); ++k) t.nrows += en[k] - st[k];
        const size_t nb = std::max<size_t>(st.size(), 1) * sizeof(int32_t);
        HIPCHK(c, hipMalloc(&t.d_row, nb));
        HIPCHK(c, hipMalloc(&t.d_end, nb));
        if (!st.empty()) {
            HIPCHK(c, hipMemcpy(t.d_row, st.data(), st.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(t.d_end, en.data(), en.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        return VTK_OK;
    };
    TRY(up(bs_, be, bd, 64));
    TRY(up(is, ie, in, GMAX - bd.grid));
    return VTK_OK;
}

// Build the halo plan of a freshly uploaded CSR (indices still GLOBAL on the device), remap
// the device indices to local numbering and exchange the send lists over RCCL.
static int setup_halo(vtk_csr *A) {
    vtk_ctx *c = A->ctx;
    const int W = c->world;
    // the indices may still be in flight on the context's (non-blocking) stream (device
    // assembly): hipMemcpy on the null stream does not wait for it
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> idx((size_t)A->nnz);
    if (A->nnz) HIPCHK(c, hipMemcpy(idx.data(), A->d_indices, A->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    int64_t nh = 0;
    if (vtk_halo_plan(A->n_global, A->offsets.data(), W, c->rank, A->nnz, idx.data(), nullptr, &nh,
                      nullptr, nullptr) != VTK_OK)
        return fail(c, VTK_ERR_ARG, context_free_error());
    A->halo_cols.resize((size_t)nh);
    A->recv_cnt.assign(W, 0);
    if (vtk_halo_plan(A->n_global, A->offsets.data(), W, c->rank, A->nnz, idx.data(), nullptr, &nh,
                      A->halo_cols.data(), A->recv_cnt.data()) != VTK_OK)
        return fail(c, VTK_ERR_ARG, context_free_error());
    A->n_halo = nh;
    A->row_halo.assign((size_t)A->n_local, 0);
    for (int64_t r = 0; r < A->n_local; ++r)
        for (int32_t k = A->h_indptr[r]; k < A->h_indptr[r + 1]; ++k)
            if (idx[k] < A->row_begin || idx[k] >= A->row_end) { A->row_halo[(size_t)r] = 1; break; }
    A->recv_off.assign(W, 0);
    for (int q = 1; q < W; ++q) A->recv_off[q] = A->recv_off[q - 1] + A->recv_cnt[q - 1];
    // remap indices on the device
    DBuf dh;
    TRY(dalloc(c, dh, (size_t)nh * sizeof(int64_t)));
    if (nh) HIPCHK(c, hipMemcpy(dh.p, A->halo_cols.data(), nh * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(c, launch_remap_cols(A->d_indices, A->nnz, A->row_begin, A->n_local, dh.as<int64_t>(), nh, c->stream));
    // counts matrix: everyone learns what it must send
    DBuf dcnt, dall;
    TRY(dalloc(c, dcnt, W * sizeof(int64_t)));
    TRY(dalloc(c, dall, (size_t)W * W * sizeof(int64_t)));
    HIPCHK(c, hipMemcpyAsync(dcnt.p, A->recv_cnt.data(), W * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    TRY(comm_allgather_i64(c, dcnt.as<int64_t>(), dall.as<int64_t>(), W));
    std::vector<int64_t> all((size_t)W * W);
    HIPCHK(c, hipMemcpyAsync(all.data(), dall.p, all.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    A->send_cnt.assign(W, 0);
    A->send_off.assign(W, 0);
    for (int q = 0; q < W; ++q) A->send_cnt[q] = all[(size_t)q * W + c->rank];
    for (int q = 1; q < W; ++q) A->send_off[q] = A->send_off[q - 1] + A->send_cnt[q - 1];
    A->n_send = W ? A->send_off[W - 1] + A->send_cnt[W - 1] : 0;
    // exchange the requested global ids
    DBuf dreq, dsend;
    TRY(dalloc(c, dreq, (size_t)nh * sizeof(int64_t)));
    TRY(dalloc(c, dsend, (size_t)A->n_send * sizeof(int64_t)));
    if (nh) HIPCHK(c, hipMemcpyAsync(dreq.p, A->halo_cols.data(), nh * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    // requests travel opposite to the data: send my recv list to each owner
    TRY(comm_alltoallv(c, dreq.p, A->recv_cnt, A->recv_off, dsend.p, A->send_cnt, A->send_off, ncclInt64, sizeof(int64_t)));
    std::vector<int64_t> sg((size_t)A->n_send);
    if (A->n_send) HIPCHK(c, hipMemcpyAsync(sg.data(), dsend.p, A->n_send * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> sl((size_t)A->n_send);
    for (int64_t k = 0; k < A->n_send; ++k) {
        const int64_t l = sg[k] - A->row_begin;
        if (l < 0 || l >= A->n_local) return fail(c, VTK_ERR_STATE, "halo request for a row this rank does not own");
        sl[k] = (int32_t)l;
    }
    HIPCHK(c, hipMalloc(&A->d_send_idx, std::max<int64_t>(1, A->n_send) * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&A->d_send_buf, std::max<int64_t>(1, A->n_send) * sizeof(double)));
    HIPCHK(c, hipMalloc(&A->d_halo, std::max<int64_t>(1, nh) * sizeof(double)));
    if (A->n_send) HIPCHK(c, hipMemcpy(A->d_send_idx, sl.data(), A->n_send * sizeof(int32_t), hipMemcpyHostToDevice));
    return VTK_OK;
}

static void free_pack(vtk_csr *A) {
    (void)hipFree(A->sell.d_pk);
    (void)hipFree(A->sell.d_pkoff);
    (void)hipFree(A->sell.d_dict);
    A->sell.d_pk = nullptr;
    A->sell.d_pkoff = nullptr;
    A->sell.d_dict = nullptr;
    A->sell.n_wide = 0;
}

static void free_sell(vtk_csr *A) {
    free_pack(A);
    (void)hipFree(A->sell.d_off);
    (void)hipFree(A->sell.d_col);
    (void)hipFree(A->sell.d_val);
    A->sell = Sell{};
    A->use_sell = false;
}

// SELL-64 copy of the (local-index) CSR on the device.  only_if_compact: stop after the
// widths when the padding would exceed 25 % of nnz (AUTO); *built says whether it exists.
static int build_sell(vtk_csr *A, bool only_if_compact, bool *built) {
    vtk_ctx *c = A->ctx;
    *built = A->sell.d_col != nullptr;
    if (*built) return VTK_OK;
    const int64_t n = A->n_local, nch = (n + 63) / 64;
    const size_t scan_bytes = std::max<size_t>(sell_scan_bytes(n), 16);
    DBuf tmp, scan;
    TRY(dalloc(c, tmp, (size_t)(nch + 1) * sizeof(int64_t)));
    TRY(dalloc(c, scan, scan_bytes));
    Sell sl;
    HIPCHK(c, hipMalloc(&sl.d_off, (size_t)(nch + 1) * sizeof(int64_t)));
    auto drop = [&]() { (void)hipFree(sl.d_off); (void)hipFree(sl.d_col); (void)hipFree(sl.d_val); };
    hipError_t e = launch_sell_build(A->d_indptr, A->d_indices, A->d_data, A->fp32, n, sl.d_off, tmp.as<int64_t>(),
                                     scan.p, scan_bytes, nullptr, nullptr, 0, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&sl.entries, sl.d_off + nch, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { drop(); return fail(c, VTK_ERR_HIP, std::string("SELL build: ") + hipGetErrorString(e)); }
    // nearly uniform widths (the 4D operator: a few chunks of 64 velocity-boundary rows are one
    // entry narrower) are padded to the widest chunk when that costs <= 2 % more entries: every
    // chunk's offset is then 64 W q and the kernels take the compile-time-width path (no offset
    // loads at the head of each chunk)
    if (nch > 0) {
        std::vector<int64_t> off((size_t)nch + 1);
        e = hipMemcpy(off.data(), sl.d_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) { drop(); return fail(c, VTK_ERR_HIP, std::string("SELL build: ") + hipGetErrorString(e)); }
        int64_t wmax = 0;
        for (int64_t q = 0; q < nch; ++q) wmax = std::max(wmax, (off[(size_t)q + 1] - off[(size_t)q]) >> 6);
        const int64_t uni = nch * 64 * wmax;
        if (wmax > 0 && uni != sl.entries && (double)uni <= 1.02 * (double)sl.entries) {
            for (int64_t q = 0; q <= nch; ++q) off[(size_t)q] = 64 * wmax * q;
            e = hipMemcpy(sl.d_off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) { drop(); return fail(c, VTK_ERR_HIP, std::string("SELL build: ") + hipGetErrorString(e)); }
            sl.entries = uni;
        }
    }
    if (only_if_compact && (double)sl.entries > 1.25 * (double)A->nnz + 64.0) { drop(); return VTK_OK; }
    const size_t vb = A->fp32 ? 4 : 8;
    e = hipMalloc(&sl.d_col, (size_t)std::max<int64_t>(sl.entries, 1) * 4);
    if (e == hipSuccess) e = hipMalloc(&sl.d_val, (size_t)std::max<int64_t>(sl.entries, 1) * vb);
    if (e == hipErrorOutOfMemory && only_if_compact) { (void)hipGetLastError(); drop(); return VTK_OK; }
    if (e == hipSuccess) e = launch_sell_build(A->d_indptr, A->d_indices, A->d_data, A->fp32, n, sl.d_off, nullptr,
                                               nullptr, 0, sl.d_col, sl.d_val, 1, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { drop(); return fail(c, e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP,
                                              std::string("SELL build: ") + hipGetErrorString(e)); }
    sl.nch = nch;
    // uniform chunk width (the Vlasov operators: every 64-row chunk holds a full-stencil row)
    {
        std::vector<int64_t> off((size_t)nch + 1);
        if (hipMemcpy(off.data(), sl.d_off, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost) == hipSuccess && nch > 0) {
            const int64_t w0 = (off[1] - off[0]) >> 6;
            bool uni = w0 > 0 && w0 < (1 << 20);
            for (int64_t q = 1; q < nch && uni; ++q) uni = ((off[(size_t)q + 1] - off[(size_t)q]) >> 6) == w0;
            sl.uniform_w = uni ? (int)w0 : 0;
        }
    }
    A->sell = sl;
    *built = true;
    return VTK_OK;
}

// Dictionary-coded columns of the SELL copy (k_sell_pack); the int32 columns stay for the
// chunks with too many distinct offsets.  Best effort: out of memory leaves the copy unpacked.
static int build_pack(vtk_csr *A) {
    vtk_ctx *c = A->ctx;
    Sell &sl = A->sell;
    if (sl.d_pk || !sl.d_col) return VTK_OK;
    const int64_t nch = sl.nch;
    const size_t scan_bytes = std::max<size_t>(sell_scan_bytes(A->n_local), 16);
    DBuf tmp, scan, cnt;
    TRY(dalloc(c, tmp, (size_t)(nch + 1) * sizeof(int64_t)));
    TRY(dalloc(c, scan, scan_bytes));
    TRY(dalloc(c, cnt, 2 * sizeof(unsigned long long)));
    int64_t words = 0;
    unsigned long long wide[2] = {0, 0};
    hipError_t e = hipMalloc(&sl.d_pkoff, (size_t)(nch + 1) * sizeof(int64_t));
    if (e == hipSuccess) e = launch_sell_pack(sl.d_off, nch, sl.d_pkoff, tmp.as<int64_t>(), scan.p, scan_bytes, nullptr,
                                              nullptr, nullptr, nullptr, 0, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&words, sl.d_pkoff + nch, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMalloc(&sl.d_pk, (size_t)std::max<int64_t>(words, 1) * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&sl.d_dict, (size_t)std::max<int64_t>(nch, 1) * 16 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, 2 * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = launch_sell_pack(sl.d_off, nch, sl.d_pkoff, nullptr, nullptr, 0, sl.d_col, sl.d_pk,
                                              sl.d_dict, cnt.as<unsigned long long>(), 1, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(wide, cnt.p, sizeof(wide), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); free_pack(A); return VTK_OK; }
    if (e != hipSuccess) { free_pack(A); return fail(c, VTK_ERR_HIP, std::string("SELL pack: ") + hipGetErrorString(e)); }
    sl.n_wide = (int64_t)wide[0];
    sl.wide_entries = (int64_t)wide[1];
    sl.pk_words = words;
    return VTK_OK;
}

static int upload_groups(vtk_ctx *c, const std::vector<int32_t> &list, int gmax, Groups &g) {
    (void)hipFree(g.d_list);
    g.d_list = nullptr;
    g.count = (int)list.size();
    g.grid = std::max(1, std::min(g.count, gmax));
    HIPCHK(c, hipMalloc(&g.d_list, std::max<size_t>(list.size(), 1) * sizeof(int32_t)));
    if (!list.empty()) HIPCHK(c, hipMemcpy(g.d_list, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return VTK_OK;
}

// groups of 4 chunks (256 rows); world > 1: interior groups (no row reads a halo column) and
// boundary groups for the overlapped exchange (grids <= 64 and the rest of GMAX)
static int build_groups(vtk_csr *A) {
    vtk_ctx *c = A->ctx;
    const int ng = (int)((A->n_local + 255) / 256);
    A->g_all.count = ng;
    A->g_all.grid = grid_for(c, std::max(1, std::min(ng, GMAX)));
    if (c->dist && A->row_halo.size() == (size_t)A->n_local) {
        std::vector<int32_t> gi, gb;
        for (int g = 0; g < ng; ++g) {
            bool h = false;
            for (int64_t r = 256 * (int64_t)g; r < std::min<int64_t>(A->n_local, 256 * (int64_t)g + 256) && !h; ++r)
                h = A->row_halo[(size_t)r] != 0;
            (h ? gb : gi).push_back(g);
        }
        TRY(upload_groups(c, gb, 64, A->g_bd));
        TRY(upload_groups(c, gi, GMAX - A->g_bd.grid, A->g_in));
    }
    return VTK_OK;
}

int apply_layout(vtk_csr *A, int layout) {
    if (layout == VTK_LAYOUT_CSR) {
        free_sell(A);
    } else {
        bool built = false;
        TRY(build_sell(A, layout == VTK_LAYOUT_AUTO, &built));
        A->use_sell = built;
        if (built && !A->g_all.grid) TRY(build_groups(A));
        if (built && layout == VTK_LAYOUT_SELL32) free_pack(A);
        else if (built) TRY(build_pack(A));
    }
    A->layout = layout;
    return VTK_OK;
}

int finish_csr(vtk_csr *A) {
    vtk_ctx *c = A->ctx;
    if (c->dist) TRY(setup_halo(A));
    TRY(upload_tiles(c, A->h_indptr, 1, A->tiles));
    TRY(build_groups(A));
    TRY(apply_layout(A, VTK_LAYOUT_AUTO));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return VTK_OK;
}

int check_partition(vtk_ctx *c, int64_t n_global, const int64_t *offsets, std::vector<int64_t> &out) {
    out.resize(c->world + 1);
    if (c->world == 1) {
        out[0] = 0;
        out[1] = n_global;
        if (offsets && (offsets[0] != 0 || offsets[1] != n_global)) return fail(c, VTK_ERR_ARG, "offsets must be {0, n}");
        return VTK_OK;
    }
    if (!offsets) return fail(c, VTK_ERR_ARG, "offsets required when world > 1");
    for (int q = 0; q <= c->world; ++q) out[q] = offsets[q];
    if (out[0] != 0 || out[c->world] != n_global) return fail(c, VTK_ERR_ARG, "offsets must span [0, n)");
    for (int q = 0; q < c->world; ++q)
        if (out[q + 1] < out[q]) return fail(c, VTK_ERR_ARG, "offsets must be non-decreasing");
    return VTK_OK;
}

void destroy_csr(vtk_csr *A) {
    if (!A) return;
    (void)hipSetDevice(A->device);
    (void)hipFree(A->d_indptr);
    (void)hipFree(A->d_indices);
    (void)hipFree(A->d_data);
    (void)hipFree(A->tiles.d_row);
    (void)hipFree(A->d_halo);
    (void)hipFree(A->d_send_idx);
    (void)hipFree(A->d_send_buf);
    (void)hipFree(A->d_lsv);
    (void)hipFree(A->d_g4tab);
    (void)hipFree(A->d_g4D);
    free_sell(A);
    (void)hipFree(A->g_in.d_list);
    (void)hipFree(A->g_bd.d_list);
    delete A;
}

// line-band structure check (vtk_csr_set_line_band): VTK_OK when every column of every row lies
// in the lines x-1..x+1 (mod X) of the row's line; VTK_ERR_ARG (no error text) otherwise
// Distributed operators (world > 1, or a one-rank communicator): the slab must hold whole lines
// and its halo must be exactly the two neighbour lines (left: the line before the slab, right: the
// one after it, periodic); the per-step ghost exchange layout is derived here
// into `out`, which the caller commits only once the whole check has passed.
struct BandLayout {
    int lblk = 0;
    int xord = 0;   // bit 0: the slab starts at global line 0, bit 1: it ends at the last line
    int peer[2] = {-1, -1};
    std::vector<int64_t> scnt, soff, rcnt, roff;
    int64_t off_first = -1, off_last = -1, off_left = -1, off_right = -1;
};

static int band_check_dist(vtk_csr *A, int64_t L, bool &solo, BandLayout &out) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local, Xg = A->n_global / L;
    solo = A->n_halo == 0 && A->n_send == 0;
    if (solo) return VTK_OK;   // no neighbour: the one-rank form (periodic wrap inside the slab)
    if (A->n_global % L != 0 || A->row_begin % L != 0 || n < 2 * L || A->n_halo != 2 * L) return VTK_ERR_ARG;
    const int64_t left = (A->row_begin / L - 1 + Xg) % Xg, right = (A->row_end / L) % Xg;
    if (left == right) return VTK_ERR_ARG;
    int64_t gl[2];
    for (int b = 0; b < 2; ++b) {
        gl[b] = A->halo_cols[(size_t)b * L] / L;
        for (int64_t v = 0; v < L; ++v)
            if (A->halo_cols[(size_t)(b * L + v)] != gl[b] * L + v) return VTK_ERR_ARG;
    }
    if (!((gl[0] == left && gl[1] == right) || (gl[0] == right && gl[1] == left))) return VTK_ERR_ARG;
    out.lblk = gl[0] == left ? 0 : 1;
    out.xord = (A->row_begin == 0 ? 1 : 0) | (A->row_end == A->n_global ? 2 : 0);
    auto owner = [&](int64_t line) {
        for (int q = 0; q < c->world; ++q)
            if (A->offsets[q] <= line * L && line * L < A->offsets[q + 1]) return q;
        return -1;
    };
    const int pl = owner(left), pr = owner(right);
    if (pl < 0 || pr < 0 || pl == c->rank || pr == c->rank) return VTK_ERR_ARG;
    out.peer[0] = pl;
    out.peer[1] = pr;
    // per peer: sends [my last line if it is my right neighbour][my first line if it is my left],
    // receives [into the left ghost if it is my left neighbour][into the right ghost if my right]:
    // a pair that is both (two ranks) matches last line -> left ghost, first line -> right ghost
    const int W = c->world;
    out.scnt.assign(W, 0);
    out.soff.assign(W, 0);
    out.rcnt.assign(W, 0);
    out.roff.assign(W, 0);
    int64_t so = 0, ro = 0;
    for (int q = 0; q < W; ++q) {
        out.soff[q] = so;
        out.roff[q] = ro;
        if (q == pr) { out.off_last = so; so += BAND_GHOST_VECS * L; }
        if (q == pl) { out.off_first = so; so += BAND_GHOST_VECS * L; }
        if (q == pl) { out.off_left = ro; ro += BAND_GHOST_VECS * L; }
        if (q == pr) { out.off_right = ro; ro += BAND_GHOST_VECS * L; }
        out.scnt[q] = so - out.soff[q];
        out.rcnt[q] = ro - out.roff[q];
    }
    return VTK_OK;
}

// local check of line length L (no collective): on success `out` holds the layout and the
// v-locality / ghost flags for band_check_all to commit
struct BandCheck {
    BandLayout lay;
    bool vloc = false, ghost = false;
};

static int band_check(vtk_csr *A, int64_t L, BandCheck &out) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local;
    // the structure only: whole lines, >= 2 of them, rows and the two halo lines within the
    // kernels' 32-bit indices.  Whether the band STEP can run on it (line parts of <= 400 rows,
    // multiples of 8: vtk_line_band_plan) is run_gmres's decision; the line path's table SpMV and
    // the SELL launches need the structure alone.
    if (L <= 0 || n <= 0 || n % L != 0 || n / L < 2 || n + 2 * L >= INT32_MAX / 2) return VTK_ERR_ARG;
    bool solo = true;
    if (c->dist && band_check_dist(A, L, solo, out.lay) != VTK_OK) return VTK_ERR_ARG;
    if (solo && n / L < 3) return VTK_ERR_ARG;
    DBuf bad;
    TRY(dalloc(c, bad, sizeof(int)));
    HIPCHK(c, hipMemsetAsync(bad.p, 0, sizeof(int), c->stream));
    if (solo) HIPCHK(c, launch_band_check(A->d_indptr, A->d_indices, n, (int)L, (int)(n / L), bad.as<int>(), c->stream));
    else HIPCHK(c, launch_band_check_dist(A->d_indptr, A->d_indices, n, (int)L, out.lay.lblk, bad.as<int>(), c->stream));
    int hb = 1;
    TRY(read_back(c, hb, bad.p));
    if (hb & 1) return VTK_ERR_ARG;
    out.vloc = (hb & 2) == 0;
    out.ghost = !solo;
    return VTK_OK;
}

// the operator's line-separable tables replaced by the ones in `lsv` (ok), or dropped
static void commit_lsv(vtk_csr *A, DBuf &lsv, bool ok, bool canon) {
    (void)hipFree(A->d_lsv);
    A->d_lsv = ok ? lsv.as<double>() : nullptr;
    A->lsv_canon = ok && canon;
    if (ok) lsv.p = nullptr;   // owned by the operator now
}

// band_check on every rank, then one agreement: the line band is set on all ranks or on none
// (collective when the context is distributed).  VTK_OK: set; VTK_ERR_ARG: not a line-band
// operator on some rank; other codes: a HIP / communicator failure on this rank.
int band_check_all(vtk_csr *A, int64_t L) {
    vtk_ctx *c = A->ctx;
    BandCheck chk;
    int rc = band_check(A, L, chk);
    // line-separable values (rank-local: the kernels read them or the SELL values, the same bits
    // either way): built into a scope-owned buffer and checked against the CSR bit for bit;
    // committed below together with the layout only once every rank has passed
    DBuf lsv;
    bool lsv_ok = false, canon = false;
    const int64_t n = A->n_local;
    if (rc == VTK_OK && !A->fp32) {
        const size_t nl = (size_t)n + 2 * (size_t)L + 2 * (size_t)(n / L);
        DBuf bad;
        rc = dalloc(c, lsv, nl * sizeof(double));
        if (rc == VTK_OK) rc = dalloc(c, bad, sizeof(int));
        int hb = 1;
        hipError_t e = hipSuccess;
        if (rc == VTK_OK) e = hipMemsetAsync(lsv.p, 0, nl * sizeof(double), c->stream);
        if (rc == VTK_OK && e == hipSuccess) e = hipMemsetAsync(bad.p, 0, sizeof(int), c->stream);
        if (rc == VTK_OK && e == hipSuccess)
            e = launch_lsv_build(A->d_indptr, A->d_indices, static_cast<const double *>(A->d_data), n, (int)L,
                                 chk.ghost ? chk.lay.lblk : -1, chk.ghost ? chk.lay.xord : 0, lsv.as<double>(), bad.as<int>(),
                                 c->stream);
        if (rc == VTK_OK && e == hipSuccess) e = hipMemcpyAsync(&hb, bad.p, sizeof(int), hipMemcpyDeviceToHost, c->stream);
        if (rc == VTK_OK && e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (rc == VTK_OK && e != hipSuccess)
            rc = fail(c, e == hipErrorOutOfMemory ? VTK_ERR_NOMEM : VTK_ERR_HIP, std::string("line values: ") + hipGetErrorString(e));
        lsv_ok = rc == VTK_OK && (hb & 1) == 0;
        canon = lsv_ok && (hb & 2) == 0;
    }
    if (c->dist) {
        // the agreement runs even after a local failure: every rank joins the same collective
        double mine = rc == VTK_OK ? 0.0 : 1.0, bad = 0.0;
        HIPCHK(c, hipMemcpyAsync(&c->d_scal[DC_NQ + 2], &mine, sizeof(double), hipMemcpyHostToDevice, c->stream));
        TRY(comm_allreduce(c, &c->d_scal[DC_NQ + 2], 1));
        TRY(read_back(c, bad, &c->d_scal[DC_NQ + 2]));
        if (rc == VTK_OK && bad != 0.0) rc = VTK_ERR_ARG;
    }
    if (rc != VTK_OK) return rc;
    // every rank passed: commit the layout and the tables (band_L is set by the caller)
    A->band_vloc = chk.vloc;
    A->band_ghost = chk.ghost;
    A->band_lblk = chk.lay.lblk;
    A->band_xord = chk.ghost ? chk.lay.xord : 0;
    A->band_peer[0] = chk.lay.peer[0];
    A->band_peer[1] = chk.lay.peer[1];
    A->band_scnt = chk.lay.scnt;
    A->band_soff = chk.lay.soff;
    A->band_rcnt = chk.lay.rcnt;
    A->band_roff = chk.lay.roff;
    A->band_off_first = chk.lay.off_first;
    A->band_off_last = chk.lay.off_last;
    A->band_off_left = chk.lay.off_left;
    A->band_off_right = chk.lay.off_right;
    commit_lsv(A, lsv, lsv_ok, canon);
    return VTK_OK;
}

// Line length the drop-in path (vtk_csr_create) tries: the smallest column distance > 1
// (periodic in n) that the first and the last local row both couple to -- for the 2D Vlasov
// operators Nv, their x-neighbour couplings (row = x Nv + v).  0 when there is none.  Collective
// (world > 1): the ranks' candidates must agree, else 0 everywhere.
static int line_len_candidate(vtk_csr *A, int64_t &L) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local, N = A->n_global;
    L = 0;
    // the local candidate; a HIP failure here votes "no candidate" (-1) instead of returning, so
    // that every rank still joins the allgather below
    auto local = [&]() -> int {
        std::vector<int64_t> d[2];
        if (n < 1) return VTK_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int s = 0; s < 2; ++s) {
            const int64_t r = s == 0 ? 0 : n - 1;
            const int32_t k0 = A->h_indptr[(size_t)r], k1 = A->h_indptr[(size_t)r + 1];
            std::vector<int32_t> idx((size_t)std::max(0, k1 - k0));
            if (k1 > k0) HIPCHK(c, hipMemcpy(idx.data(), A->d_indices + k0, (k1 - k0) * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (int32_t l : idx) {
                const int64_t g = l < n ? l + A->row_begin : A->halo_cols[(size_t)(l - n)];
                int64_t dist = std::llabs(g - (A->row_begin + r));
                dist = std::min(dist, N - dist);
                if (dist > 1) d[s].push_back(dist);
            }
            std::sort(d[s].begin(), d[s].end());
        }
        for (int64_t v : d[0])
            if (std::binary_search(d[1].begin(), d[1].end(), v)) { L = v; break; }
        return VTK_OK;
    };
    const int lrc = local();
    if (lrc != VTK_OK) L = -1;
    if (c->dist && c->world > 120) {
        // the agreement below gathers into the context's scalar scratch (room for 120 ranks, no
        // allocation that could fail on one rank only).  Beyond that every rank
        // skips the detection alike -- no collective, the plain path; vtk_csr_set_line_band
        // still sets the band explicitly
        L = 0;
        return lrc;
    }
    if (c->dist) {
        const int W = c->world;
        int64_t *mine = reinterpret_cast<int64_t *>(c->d_scal + 128);
        HIPCHK(c, hipMemcpyAsync(mine, &L, sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        TRY(comm_allgather_i64(c, mine, mine + 1, 1));
        std::vector<int64_t> h((size_t)W);
        HIPCHK(c, hipMemcpyAsync(h.data(), mine + 1, W * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int64_t v : h)
            if (v != h[0]) { L = 0; break; }
        if (L != 0) L = h[0];
    }
    if (L < 0) L = 0;
    return lrc;
}

// the operator's 4D grid tables replaced by (tab, D) of geometry g, or (tab null) dropped
void set_grid4_tables(vtk_csr *A, Grid4 g, DBuf *tab, DBuf *D) {
    (void)hipFree(A->d_g4tab);
    (void)hipFree(A->d_g4D);
    g.tab = A->d_g4tab = tab ? tab->as<double>() : nullptr;
    g.D = A->d_g4D = tab ? D->p : nullptr;
    if (tab) tab->p = D->p = nullptr;   // owned by the operator now
    A->g4 = g;
}

// 4D grid structure (vtk::Grid4): tables built and every entry checked on the device; rank-local
// (the kernels read the tables or the SELL copy, the same bits either way: no agreement needed).
// VTK_ERR_ARG when the operator is not such a grid (the state is then unchanged).
int grid4_set(vtk_csr *A, int64_t Ny, int64_t Nvx, int64_t Nvy) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local, S4 = Ny * Nvx * Nvy;
    if (Ny < 3 || Nvx < 2 || Nvy < 2 || S4 <= 0 || S4 > INT32_MAX || n <= 0 || n % S4 != 0 || A->n_global % S4 != 0 ||
        n + 2 * S4 >= INT32_MAX / 2)
        return VTK_ERR_ARG;
    Grid4 g;
    g.Ny = (int)Ny;
    g.Nvx = (int)Nvx;
    g.Nvy = (int)Nvy;
    g.X = (int)(n / S4);
    if (c->dist) {   // across ranks: whole x planes, the halo = the two neighbour planes
        bool solo = true;
        BandLayout lay;
        if (band_check_dist(A, S4, solo, lay) != VTK_OK) return VTK_ERR_ARG;
        if (!solo) {
            g.lblk = lay.lblk;
            g.xord = (A->row_begin == 0 ? 1 : 0) | (A->row_end == A->n_global ? 2 : 0);
        }
    }
    if (g.lblk < 0 && g.X < 3) return VTK_ERR_ARG;
    A->g4_try = g;   // the geometry a value update checks its new values against (update_finish)
    DBuf tab, D, bad;
    TRY(dalloc(c, tab, grid4_tab_len(g) * sizeof(double)));
    TRY(dalloc(c, D, (size_t)n * (A->fp32 ? 4 : 8)));
    TRY(dalloc(c, bad, sizeof(int)));
    HIPCHK(c, hipMemsetAsync(tab.p, 0, grid4_tab_len(g) * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(bad.p, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_grid4_build(A->d_indptr, A->d_indices, A->d_data, A->fp32, n, g, tab.as<double>(), D.p,
                                 bad.as<int>(), c->stream));
    int hb = 1;
    TRY(read_back(c, hb, bad.p));
    if (hb != 0) return VTK_ERR_ARG;
    set_grid4_tables(A, g, &tab, &D);
    return VTK_OK;
}

// the drop-in path's 4D grid detection: the distinct column distances of the first local row
// (periodic in n) are 1, Nvy, Nvx Nvy, Ny Nvx Nvy for the 4D Vlasov operators (0: no candidate)
static int grid4_candidate(vtk_csr *A, int64_t &Ny, int64_t &Nvx, int64_t &Nvy) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local, N = A->n_global;
    Ny = Nvx = Nvy = 0;
    if (n < 1) return VTK_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int32_t k0 = A->h_indptr[0], k1 = A->h_indptr[1];
    if (k1 - k0 < 5 || k1 - k0 > 64) return VTK_OK;
    std::vector<int32_t> idx((size_t)(k1 - k0));
    HIPCHK(c, hipMemcpy(idx.data(), A->d_indices + k0, (k1 - k0) * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> d;
    for (int32_t l : idx) {
        const int64_t g = l < n ? l + A->row_begin : A->halo_cols[(size_t)(l - n)];
        int64_t dist = std::llabs(g - A->row_begin);
        dist = std::min(dist, N - dist);
        if (dist > 0) d.push_back(dist);
    }
    std::sort(d.begin(), d.end());
    d.erase(std::unique(d.begin(), d.end()), d.end());
    // {1, S2, S3, S4}, plus the periodic y wrap S4 - S3 (= (Ny - 1) S3) when Ny > 2
    if (d.size() < 4 || d.size() > 5 || d[0] != 1) return VTK_OK;
    const int64_t S2 = d[1], S3 = d[2], S4 = d.back();
    if (S3 % S2 != 0 || S4 % S3 != 0 || (d.size() == 5 && d[3] != S4 - S3)) return VTK_OK;
    Nvy = S2;
    Nvx = S3 / S2;
    Ny = S4 / S3;
    return VTK_OK;
}

int auto_grid4(vtk_csr *A) {
    if (!A->ctx->tune.auto_band) return VTK_OK;
    int64_t Ny, Nvx, Nvy;
    TRY(grid4_candidate(A, Ny, Nvx, Nvy));
    if (Ny <= 0) return VTK_OK;
    const int rc = grid4_set(A, Ny, Nvx, Nvy);
    // no such grid, or no memory for its tables: the operator keeps the SELL path (the detection is
    // a speed-up the drop-in CSR does not need)
    if (rc == VTK_ERR_NOMEM) A->ctx->err.clear();
    return rc == VTK_ERR_ARG || rc == VTK_ERR_NOMEM ? VTK_OK : rc;
}

// the drop-in path's line-band detection: the same check vtk_csr_set_line_band runs, on the
// candidate line length (tuning auto_band 0: off)
int auto_line_band(vtk_csr *A) {
    if (!A->ctx->tune.auto_band) return VTK_OK;
    int64_t L = 0;
    TRY(line_len_candidate(A, L));
    if (L <= 0) return VTK_OK;   // uniform across ranks: nobody enters the collective below
    const int rc = band_check_all(A, L);   // collective: every rank gets here (L agreed above)
    if (rc == VTK_OK) A->band_L = L;
    else if (rc == VTK_ERR_NOMEM) A->ctx->err.clear();   // no memory for the tables: not detected
    else if (rc != VTK_ERR_ARG) return rc;
    return VTK_OK;
}

// ---- value updates (vtk_csr_update_values / vtk_csr_update_vlasov) -----------
// What depends on the values: the CSR values, the SELL copy's values and the tables checked
// against them (line-separable values, 4D grid).  Everything else of a vtk_csr is planned from
// the pattern and stays.  update_prepare allocates all an update can need -- before the first
// overwrite, so a VTK_ERR_NOMEM return leaves the operator as it was --, the caller then writes
// the new values into d_data on the context's stream, and update_finish redoes the rest.
static size_t lsv_len(const vtk_csr *A) {
    return (size_t)A->n_local + 2 * (size_t)A->band_L + 2 * (size_t)(A->n_local / A->band_L);
}

int update_prepare(vtk_csr *A, UpdateScratch &u) {
    vtk_ctx *c = A->ctx;
    // the tables a fresh operator of this pattern would try: line values on a line band (f64),
    // the 4D grid where one was tried (present or lost to earlier values)
    u.want_lsv = A->band_L > 0 && !A->fp32;
    u.want_g4 = A->g4_try.Ny > 0;
    TRY(dalloc(c, u.bad, 2 * sizeof(int)));
    if (u.want_lsv) TRY(dalloc(c, u.lsv, lsv_len(A) * sizeof(double)));
    if (u.want_g4) {
        TRY(dalloc(c, u.g4tab, grid4_tab_len(A->g4_try) * sizeof(double)));
        TRY(dalloc(c, u.g4D, (size_t)A->n_local * (A->fp32 ? 4 : 8)));
    }
    return VTK_OK;
}

int update_finish(vtk_csr *A, UpdateScratch &u) {
    vtk_ctx *c = A->ctx;
    const int64_t n = A->n_local;
    const double vb = A->fp32 ? 4.0 : 8.0;
    const double b_csr = 4.0 * (n + 1) + (4.0 + vb) * A->nnz;   // one pass over the CSR
    HIPCHK(c, hipMemsetAsync(u.bad.p, 0, 2 * sizeof(int), c->stream));
    if (A->sell.d_val) {
        Prof pf(c, "sell_refresh", -1, vb * ((double)A->nnz + (double)A->sell.entries));
        HIPCHK(c, launch_sell_refresh(A->d_indptr, A->d_data, A->fp32, n, A->sell.d_off, A->sell.d_val, c->stream));
    }
    if (u.want_lsv) {
        HIPCHK(c, hipMemsetAsync(u.lsv.p, 0, lsv_len(A) * sizeof(double), c->stream));
        Prof pf(c, "lsv_build", -1, 2.0 * b_csr + 8.0 * (double)lsv_len(A));   // build + check passes
        HIPCHK(c, launch_lsv_build(A->d_indptr, A->d_indices, static_cast<const double *>(A->d_data), n, (int)A->band_L,
                                   A->band_ghost ? A->band_lblk : -1, A->band_ghost ? A->band_xord : 0,
                                   u.lsv.as<double>(), u.bad.as<int>(), c->stream));
    }
    if (u.want_g4) {
        HIPCHK(c, hipMemsetAsync(u.g4tab.p, 0, grid4_tab_len(A->g4_try) * sizeof(double), c->stream));
        Prof pf(c, "grid4_build", -1, 2.0 * b_csr + vb * (double)n);
        HIPCHK(c, launch_grid4_build(A->d_indptr, A->d_indices, A->d_data, A->fp32, n, A->g4_try, u.g4tab.as<double>(),
                                     u.g4D.p, u.bad.as<int>() + 1, c->stream));
    }
    int hb[2] = {1, 1};
    TRY(read_back(c, hb, u.bad.p));
    if (c->prof_on) prof_flush(c);
    // commit, as band_check_all and grid4_set do: tables that passed replace the old ones, tables
    // the new values fail are dropped (the structural band_L stays)
    if (A->band_L > 0) commit_lsv(A, u.lsv, u.want_lsv && (hb[0] & 1) == 0, (hb[0] & 2) == 0);
    if (u.want_g4) set_grid4_tables(A, hb[1] == 0 ? A->g4_try : Grid4{}, hb[1] == 0 ? &u.g4tab : nullptr, &u.g4D);
    A->values_epoch += 1;
    return VTK_OK;
}

}  // namespace vtk
