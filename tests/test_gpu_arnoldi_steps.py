"""Every Arnoldi step pinned to the extended-precision reference (oracle/arnoldi.py).

The solve-level bars cannot see a step that is wrong at the 1e-12 level: restarted GMRES repairs
it in the next cycle.  Here one restart cycle is captured on the device (``ctx.capture_arnoldi``:
V, H, S, giv, Hraw at the moment between the x update and the cycle-end residual) and measured in
longdouble against B = M^-1 A built from the downloaded CSR values:

  F1 the Arnoldi relation per column, F2 orthonormality of the final columns, F3 the cycle start
  (v_0, beta), F4 H / giv / S against a longdouble Givens QR of Hraw, F5 the x correction against
  the longdouble minimiser's, F6 the reported preconditioned residual against the true one.

Bars: each figure at most 16x the same figure of a plain float64 NumPy Arnoldi (CGS2 for the
DCGS2 paths, MGS for MGS) on the same operator, x_in and column count, computed here.  The device
sums in another fixed order through up to 1024 partials and DCGS2 forms h from lagged quantities
(one more rounding layer); 16x stays more than two orders below the smallest planted defect of
tests/test_arnoldi_reference.py.  The two figures that are errors of one float64 scalar (F3b,
F6) take their reference no lower than the number format allows (see _compare).
``maxiter=1, restart=m`` and a tolerance that cannot be met:
the cycle has exactly m columns and every step up to the top one runs.
"""
import functools
import os
import socket

import numpy as np
import pytest

from oracle import arnoldi as ar
from oracle import twin

pytestmark = pytest.mark.gpu

MARGIN = 16.0
NOSTOP = 1e-30      # rtol no cycle can meet: the cycle runs all its columns
U = 2.0 ** -53      # float64 unit roundoff
# one tenth of the smallest planted-defect figure of tests/test_arnoldi_reference.py (h_{3,11}
# scaled by 1 + 1e-10 on S2: F1 = 5.2e-13): no floor lifts a bar above it
DEFECT_CAP = 5.2e-14


# ---- host side: operators, reference runs, the comparison ----------------------------------
class _Ops:
    """The longdouble and float64 operators of one (CSR, preconditioner), built once."""

    def __init__(self, csr, n, prec):
        ip, ix, d = csr
        self.csr, self.n = csr, n
        self.ld = ar.Operator(ip, ix, d, n, prec)
        self.f64 = ar.Operator(ip, ix, d, n, prec, np.float64)


def _cycle_of(cap, x_out, presid):
    """The device capture as the record the figures read."""
    early = {}
    if cap.Hraw is not None and cap.xup_tag >= 0 and cap.xup_tag == cap.stop_col:
        early[cap.stop_col] = cap.nu      # the stop column was committed from its tentative form
    return ar.Cycle(V=cap.V, cols=cap.cols, final_cols=cap.final_cols, x_in=cap.x_in, x_out=x_out, H=cap.H,
                    S=cap.S, giv=cap.giv, presid=presid, Hraw=cap.Hraw, early=early)


def _compare(tag, ops, b, cyc, scheme, which=("F1", "F2", "F3v", "F3b", "F4", "F4e", "F5", "F6")):
    """Device figures against the float64 reference's on the same x_in and column count."""
    delta = ar.minimiser(ops.ld, b, cyc.x_in, cyc.cols)
    fd = ar.figures(ops.ld, b, cyc, delta)
    dev = ar.worst(fd)
    ref = ar.worst(ar.figures(ops.ld, b, ar.run_cycle(ops.f64, b, cyc.x_in, cyc.cols, scheme), delta))
    if cyc.early:   # a column committed from its tentative form (early commit), apart from the exact ones
        dev["F4e"] = max(fd["F4"][c] for c in cyc.early)
        dev["F4"] = max([f for c, f in enumerate(fd["F4"]) if c not in cyc.early], default=0.0)
        ref["F4e"] = ref["F4"]
    # F3b and F6 are relative errors of ONE float64 scalar: the reference's own value is a single
    # rounding draw and falls as low as 2e-18, below what storing the scalar in float64 allows.
    # Their reference figure is floored at the format's unit roundoff U -- for F6 times
    # beta / presid, both from the longdouble minimiser: presid = ||r_in - B delta|| is the
    # difference of two vectors of norm ~beta, each carrying U beta of rounding -- and the floor
    # never lifts the bar above one tenth of the smallest planted-defect figure.
    xin = np.asarray(cyc.x_in).astype(ar.LD)
    r_in, r_out = ops.ld.presidual(b, xin), ops.ld.presidual(b, xin + delta)
    amp = float(np.sqrt(r_in @ r_in) / np.sqrt(r_out @ r_out))
    floor = {"F3b": U, "F6": min(U * amp, DEFECT_CAP / MARGIN)}
    bad = []
    for k in which:
        if k not in dev:
            continue
        r_eff = max(ref[k], floor.get(k, 0.0))
        ratio = dev[k] / r_eff if r_eff > 0 else (0.0 if dev[k] == 0 else np.inf)
        print(f"ARN|{tag}|{scheme}|k={cyc.cols} fin={cyc.final_cols}|{k}|dev {dev[k]:.3e}|ref {ref[k]:.3e}|"
              f"floor {floor.get(k, 0.0):.3e}|x{ratio:.2f}")
        if not dev[k] <= MARGIN * r_eff:
            bad.append((k, dev[k], ref[k], ratio))
    assert not bad, (tag, bad)
    return dev, ref


def _run(vk, gpu, A, M, b, m, *, x0=None, rtol=NOSTOP, maxiter=1, cycle=0, orth=None):
    with gpu.capture_arnoldi(cycle):
        x, info = vk.gmres(A, b, x0=x0, rtol=rtol, M=M, restart=m, maxiter=maxiter, orth=orth)
    st = vk.last_stats()
    cap = vk.last_arnoldi(gpu)
    assert cap.cycle == st.restarts - 1, "the captured cycle is not the solve's last: x is not its x_out"
    assert cap.restart == min(m, A.n_local) and cap.n_local == A.n_local
    return _cycle_of(cap, x, st.presid), cap, st


def _check_full_cycle(cap, m, dc=True):
    """A cycle that ran out of columns: m committed; which columns of V are final (vtkrylov.h)."""
    assert cap.cols == m and cap.breakdown == 0
    if dc:
        assert cap.final_cols == (m if cap.xup_tag < 0 else max(cap.xup_tag, 1)), (cap.final_cols, cap.xup_tag)
        assert cap.final_cols >= m - 1
    else:
        assert cap.final_cols == m + 1


@functools.lru_cache(maxsize=None)
def _rhs(n):
    return twin.rhs(n)


# ---- 2D operators: band step ----------------------------------------------------------------
class _Case2D:
    def __init__(self, vk, gpu, shape, bs=8, mode="auto", layout=None):
        self.vk, self.gpu = vk, gpu
        self.A = vk.vlasov_operator(vk.vlasov_params(2, shape), ctx=gpu)
        if layout:
            self.A.set_layout(layout)
        self.M = vk.block_jacobi(self.A, bs, mode=mode) if bs else None
        self.n = shape[0] * shape[1]
        self.b = _rhs(self.n)
        self.ops = _Ops(self.A.download(), self.n, ("bj", bs) if bs else None)

    def close(self):
        if self.M:
            self.M.close()
        self.A.close()


@pytest.fixture(scope="module")
def s2(vk_lib, gpu):
    c = _Case2D(vk_lib, gpu, twin.CONFIGS["S2"].shape)
    yield c
    c.close()


def _band(c, m, tag, band=1, **tune):
    with c.gpu.tuning(band_long_rows=0, **tune):
        cyc, cap, st = _run(c.vk, c.gpu, c.A, c.M, c.b, m)
    assert st.band == band == cap.band and st.orth == 1, (tag, st.band)
    _check_full_cycle(cap, m)
    _compare(tag, c.ops, c.b, cyc, "cgs2")
    return cap


@pytest.mark.parametrize("m", list(range(2, 21)))
def test_band_step_every_restart(s2, m):
    """Default band_opt with bits 3, 4 and the J > 12 prefetch live: every top step 0..m-1."""
    _band(s2, m, f"band S2 m={m}")


@pytest.mark.parametrize("opt", [0, 1, 2, 3, 63, 95, None])
def test_band_step_variants(s2, opt):
    tune = {} if opt is None else {"band_opt": opt}
    _band(s2, 20, f"band S2 m=20 opt={opt}", **tune)


@pytest.mark.parametrize("m", [3, 14, 20])
@pytest.mark.parametrize("shape", [(48, 8), (40, 816), (24, 1000)])
def test_band_step_line_lengths(vk_lib, gpu, shape, m):
    c = _Case2D(vk_lib, gpu, shape)
    try:
        _band(c, m, f"band {shape} m={m}")
    finally:
        c.close()


@pytest.mark.parametrize("Nv", [32, 800])
@pytest.mark.parametrize("Nx", [3, 4, 7])
def test_band_step_few_lines(vk_lib, gpu, Nx, Nv):
    c = _Case2D(vk_lib, gpu, (Nx, Nv))
    try:
        _band(c, 20, f"band ({Nx},{Nv}) m=20")
    finally:
        c.close()


# ---- cycle start ----------------------------------------------------------------------------
@pytest.mark.parametrize("band", [1, 0])
@pytest.mark.parametrize("ring", [0, 1, 64])
def test_cycle_start_after_restart(s2, ring, band):
    """Cycle 1 of a solve with x0 != 0: its v_0 comes from the cycle-end residual of cycle 0 (the
    ring epilogue that overwrites V[0]); x_in is the captured x."""
    c = s2
    x0 = twin.rhs(c.n, seed=0xB00) * 1e-3
    c.gpu.set_band(bool(band))
    try:
        with c.gpu.tuning(band_long_rows=0, cyc_ring=ring):
            cyc, cap, st = _run(c.vk, c.gpu, c.A, c.M, c.b, 5, x0=x0, maxiter=2, cycle=1)
    finally:
        c.gpu.set_band(True)
    assert cap.cycle == 1 and st.band == band
    assert not np.array_equal(cap.x_in, x0), "x_in is the solve's x0, not cycle 1's"
    _check_full_cycle(cap, 5)
    _compare(f"cycle 1 restart=5 cyc_ring={ring} band={band}", c.ops, c.b, cyc, "cgs2")


# ---- natural stop ---------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [20, 5])
def test_natural_stop(s2, restart):
    """rtol 1e-8: the last cycle stops inside a step (restart 20: 68 = 3 * 20 + 8 columns, an
    even step; restart 5: 68 = 13 * 5 + 3, a reversed one); whatever columns are final."""
    c = s2
    with c.gpu.tuning(band_long_rows=0):
        cyc, cap, st = _run(c.vk, c.gpu, c.A, c.M, c.b, restart, rtol=1e-8, maxiter=400, cycle=-2)
    assert st.band == 1 and cap.cols < restart and cap.stop_col == cap.cols - 1
    assert cap.final_cols == max(cap.xup_tag, 1) and cap.xup_tag in (cap.stop_col, cap.stop_col + 1)
    print(f"natural stop restart={restart}: cycle {cap.cycle} cols {cap.cols} final {cap.final_cols} xup {cap.xup_tag}")
    _compare(f"natural stop restart={restart}", c.ops, c.b, cyc, "cgs2", which=("F1", "F2", "F4", "F4e", "F6"))


# ---- band off: fused / split DCGS2, MGS, layouts --------------------------------------------
@pytest.fixture
def band_off(gpu):
    gpu.set_band(False)
    yield
    gpu.set_band(True)


@pytest.mark.parametrize("m", [2, 13, 20])
@pytest.mark.parametrize("kind", ["bj8-tridiag", "bj8-inverse", "bj4", "bj16", "none"])
def test_dcgs2_band_off(vk_lib, gpu, band_off, kind, m):
    bs = {"bj8-tridiag": 8, "bj8-inverse": 8, "bj4": 4, "bj16": 16, "none": 0}[kind]
    mode = kind.split("-")[1] if "-" in kind else "auto"
    c = _Case2D(vk_lib, gpu, twin.CONFIGS["S2"].shape, bs=bs, mode=mode)
    try:
        cyc, cap, st = _run(vk_lib, gpu, c.A, c.M, c.b, m, orth="dcgs2")
        assert st.band == 0 and st.orth == 1
        _check_full_cycle(cap, m)
        _compare(f"dcgs2 band off {kind} m={m}", c.ops, c.b, cyc, "cgs2")
    finally:
        c.close()


@pytest.mark.parametrize("m", [1, 20, 33])
def test_mgs(s2, band_off, m):
    c = s2
    cyc, cap, st = _run(c.vk, c.gpu, c.A, c.M, c.b, m, orth="mgs")
    assert st.orth == 0 and cap.Hraw is None
    _check_full_cycle(cap, m, dc=False)
    _compare(f"mgs m={m}", c.ops, c.b, cyc, "mgs")


@pytest.mark.parametrize("m", [2, 13, 20])
@pytest.mark.parametrize("layout", ["csr", "sell", "sell32"])
def test_dcgs2_layouts(vk_lib, gpu, band_off, layout, m):
    c = _Case2D(vk_lib, gpu, twin.CONFIGS["S2"].shape, layout=layout)
    try:
        assert c.A.layout == layout
        cyc, cap, st = _run(vk_lib, gpu, c.A, c.M, c.b, m, orth="dcgs2")
        assert st.band == 0
        _check_full_cycle(cap, m)
        _compare(f"dcgs2 layout {layout} m={m}", c.ops, c.b, cyc, "cgs2")
    finally:
        c.close()


# ---- 4D: ring step, its fall-backs, shapes past the ring's limits --------------------------
def _case4(vk, gpu, shape, fp32):
    A = vk.vlasov_operator(vk.vlasov_params(4, shape, fp32=fp32), ctx=gpu)
    M = vk.block_jacobi(A, 8)
    n = int(np.prod(shape))
    return A, M, _rhs(n), _Ops(A.download(), n, ("bj", 8))


@pytest.fixture(scope="module", params=["S4", "S4F"])
def s4(request, vk_lib, gpu):
    p = twin.CONFIGS[request.param]
    A, M, b, ops = _case4(vk_lib, gpu, p.shape, p.fp32)
    yield request.param, A, M, b, ops
    M.close()
    A.close()


@pytest.mark.parametrize("m", [2, 20])
@pytest.mark.parametrize("tune", [{}, {"g4_ring": 0}, {"c4_fused": 0}, {"grid4": 0}], ids=["ring", "g4_ring0", "c4_fused0", "grid40"])
def test_4d_steps(vk_lib, gpu, s4, tune, m):
    name, A, M, b, ops = s4
    with gpu.tuning(**tune):
        cyc, cap, st = _run(vk_lib, gpu, A, M, b, m)
    assert st.band == 0 and st.orth == 1
    _check_full_cycle(cap, m)
    _compare(f"4d {name} {tune or 'ring'} m={m}", ops, b, cyc, "cgs2")


@pytest.mark.parametrize("shape", [(520, 3, 4, 4), (3, 3, 64, 64)])
def test_4d_past_ring_limits(vk_lib, gpu, shape):
    A, M, b, ops = _case4(vk_lib, gpu, shape, False)
    try:
        cyc, cap, st = _run(vk_lib, gpu, A, M, b, 5)
        _check_full_cycle(cap, 5)
        _compare(f"4d {shape} m=5", ops, b, cyc, "cgs2")
    finally:
        M.close()
        A.close()


# ---- line Jacobi ----------------------------------------------------------------------------
LINE_M = 8   # a line-Jacobi cycle of 20 columns reaches rounding on S2: F6 would measure noise


@pytest.mark.parametrize("name,seg", [("S2", 8), ("S2", 25), ("S2", 64), ("C0", 25)])
def test_line_jacobi_steps(vk_lib, gpu, name, seg):
    """seg 8 and 25: the fused-dots sweep (with the SpMV inside on the line-separable S2); seg 64
    = all of S2's lines in one segment (the generic sweep); C0: stride 1."""
    p = twin.CONFIGS[name]
    params = vk_lib.vlasov_params(p.dim, p.shape)
    A = vk_lib.vlasov_operator(params, ctx=gpu)
    stride = vk_lib.vlasov_line_stride(params)
    M = vk_lib.line_jacobi(A, stride, seg)
    try:
        b = _rhs(p.n)
        ops = _Ops(A.download(), p.n, ("line", stride, seg))
        cyc, cap, st = _run(vk_lib, gpu, A, M, b, LINE_M)
        assert st.orth == 1 and st.band == 0
        _check_full_cycle(cap, LINE_M)
        _compare(f"line {name} seg={seg} m={LINE_M}", ops, b, cyc, "cgs2")
    finally:
        M.close()
        A.close()


# ---- the hook itself ------------------------------------------------------------------------
def test_capture_state(vk_lib, gpu, s2):
    """Nothing captured -> ERR_STATE; an unarmed solve drops an earlier capture; a chosen cycle the
    solve never reaches captures nothing."""
    c = s2
    vk_lib.gmres(c.A, c.b, rtol=1e-2, M=c.M)
    with pytest.raises(vk_lib._abi.VtkError) as e:
        vk_lib.last_arnoldi(gpu)
    assert e.value.status == vk_lib._abi.ERR_STATE
    with gpu.capture_arnoldi(0):
        x1, _ = vk_lib.gmres(c.A, c.b, rtol=1e-8, M=c.M)
    assert vk_lib.last_arnoldi(gpu).cycle == 0
    x2, _ = vk_lib.gmres(c.A, c.b, rtol=1e-8, M=c.M)      # disarmed on exit
    assert np.array_equal(x1, x2), "the capture changed the solve"
    with pytest.raises(vk_lib._abi.VtkError):
        vk_lib.last_arnoldi(gpu)
    with gpu.capture_arnoldi(50):
        vk_lib.gmres(c.A, c.b, rtol=1e-8, M=c.M)
    with pytest.raises(vk_lib._abi.VtkError):
        vk_lib.last_arnoldi(gpu)


# ---- ranks sharing the GPU (host-staged communicator) --------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, case, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    p = twin.CONFIGS[case]
    offs = vk.partition_rows(p.n, world, p.shape[-1] if p.dim == 2 else int(np.prod(p.shape[1:])))
    rb, re_ = int(offs[rank]), int(offs[rank + 1])
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=ctx, offsets=offs)
    M = vk.block_jacobi(A, 8)
    b = twin.rhs(p.n)[rb:re_]
    ctx.set_tuning("band_long_rows", 0)
    if p.dim == 4:
        ctx.set_tuning("g4_ring", 64)   # the LDS-ring step across ranks (tests/test_gpu_multirank.py)
    out = {}
    for m in (20, 3):
        ctx.profile(True)
        with ctx.capture_arnoldi(0):
            x, info = vk.gmres(A, b, rtol=NOSTOP, M=M, restart=m, maxiter=1, orth="dcgs2")
        st = vk.last_stats()
        out[f"classes_{m}"] = ",".join(sorted(k for k, e in ctx.profile_read().items() if e["launches"] > 0))
        ctx.profile(False)
        cap = vk.last_arnoldi(ctx)
        out.update({f"x_{m}": x, f"V_{m}": cap.V, f"xin_{m}": cap.x_in, f"H_{m}": cap.H, f"Hraw_{m}": cap.Hraw,
                    f"S_{m}": cap.S, f"giv_{m}": cap.giv, f"nu_{m}": cap.nu,
                    f"meta_{m}": np.array([cap.cols, cap.final_cols, cap.stop_col, cap.xup_tag, cap.cycle, st.band,
                                           cap.breakdown]),
                    f"presid_{m}": st.presid})
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("S2", 2), ("S2", 3), ("S4", 2), ("S4", 3)])
def test_steps_across_ranks(tmp_path, case, world):
    """S2: the band step with ghost lines; S4: the ring step's interior and boundary halves.  The
    small arrays are bit-identical on every rank; the figures are those of the gathered V against
    the global B."""
    import torch.multiprocessing as mp
    from types import SimpleNamespace
    mp.spawn(_worker, args=(world, _free_port(), case, str(tmp_path)), nprocs=world, join=True)
    p = twin.CONFIGS[case]
    ops = _Ops(twin.generate(p), p.n, ("bj", 8))
    b = _rhs(p.n)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    for m in (20, 3):
        for r in range(world):
            assert z[r]["errors"].size == 0, z[r]["errors"]
            for k in ("H", "Hraw", "S", "giv", "nu", "meta", "presid"):
                assert np.array_equal(z[r][f"{k}_{m}"], z[0][f"{k}_{m}"]), (k, m, r)
        cols, fin, stop_col, xup, cyc_i, band, brk = (int(v) for v in z[0][f"meta_{m}"])
        assert band == (1 if case == "S2" else 0) and cyc_i == 0
        classes = str(z[0][f"classes_{m}"]).split(",")
        assert ("band_step" if case == "S2" else "spmv_bj_bd") in classes, classes
        V = np.concatenate([z[r][f"V_{m}"] for r in range(world)], axis=1)
        cap = SimpleNamespace(V=V, cols=cols, final_cols=fin, stop_col=stop_col, xup_tag=xup, breakdown=brk,
                              x_in=np.concatenate([z[r][f"xin_{m}"] for r in range(world)]),
                              H=z[0][f"H_{m}"], Hraw=z[0][f"Hraw_{m}"], S=z[0][f"S_{m}"], giv=z[0][f"giv_{m}"],
                              nu=float(z[0][f"nu_{m}"]))
        _check_full_cycle(cap, m)
        x = np.concatenate([z[r][f"x_{m}"] for r in range(world)])
        _compare(f"ranks {case} world={world} m={m}", ops, b, _cycle_of(cap, x, float(z[0][f"presid_{m}"])), "cgs2")
