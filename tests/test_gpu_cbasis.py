"""Compressed-basis GMRES on the device (``vk.gmres(..., basis="float32")``) against
the NumPy restatement of tests/cbasis_ref.py.

Captured cycles (``rtol`` no cycle can meet, ``maxiter=1``: the cycle runs all its columns): F1-F6 of
oracle.arnoldi.figures, measured in 80-bit, each at most 16x the same figure of the restatement's
float32-basis cycle on the same operator, x_in and column count (cbasis_ref.compare prints every
figure before it asserts).  Natural stops: info, the true residual recomputed on the host, the inner
iterations within +-1 of the restatement's (under SciPy's ptol schedule, which the device runs, and
under the fixed first ptol of the iteration table in tests/test_cbasis_host.py), and x within the derived bound
    ||x - x_scipy|| <= (||r|| + ||r_scipy||) / sigma_min(A)
(x - x_scipy = A^-1 (r_scipy - r); sigma_min from a dense SVD of these small operators).

Shapes.  The kernels own four rows per thread and 1024 per workgroup: n = 1025, 1026, 1027 leave a
tail of 1, 2, 3 rows in the second workgroup, n = 1, 3, 5 a one-workgroup grid that is all tail, S2
(2048 rows) whole quads in several workgroups; restarts 1, 2, 8, 9, 16, 17, 24, 25, 32 straddle the
dots kernel's accumulator ladder (8 / 16 / 24 / 32).  Where restart >= n the Krylov space is exhausted
inside the cycle (SciPy clips restart to n) and its last column is a breakdown, which the figures do
not describe: those (n, restart) pairs run the same kernels to their natural end instead and are held
to the solve bars against the dense solution.

The restatement a device cycle is compared with is its "candidate" variant (the operator applied to
the float64 candidate, which is what the device does; cbasis_ref.DEVICE_VARIANT states why the other
variant is another algorithm at the float32 level).

Measured ratios device / restatement (MI355X; worst over each test's cases; bar 16):
                               F1    F2    F3v   F3b   F4    F4e   F5    F6
    test_row_tails             1.03  1.00  1.00  1.93  4.95  4.67  1.62  6.40
    test_several_workgroups    1.00  1.00  1.00  3.83  1.60  0.85  1.00  2.71
    test_operator_step_forms   1.00  1.00  1.00  3.59  1.50  0.97  1.00  1.07
    test_4d_steps              1.00  1.00  1.00  1.67  1.04  1.64  1.00  1.01
Natural stops: device and restatement count the same inner iterations and cycles in every case (S2
68 in 4 and 68 in 14, S4F 74 in 4 and 89 in 18, S2 / x-line 14 in 2 against 12 in 1 with the float64
basis); host-staged ranks (2 and 3, S2 and S4) count what one rank counts.
"""
import functools
import json
import os
import socket

import numpy as np
import pytest

import cbasis_ref as cr
from oracle import cases, twin

pytestmark = pytest.mark.gpu

NOSTOP = 1e-30
F32, F64 = 1, 0


@functools.lru_cache(maxsize=None)
def _rhs(n):
    return twin.rhs(n)


@functools.lru_cache(maxsize=None)
def _sigma_min(name):
    p = twin.CONFIGS[name]
    return float(np.linalg.svd(cases.dense(*twin.generate(p)), compute_uv=False)[-1])


def _run(vk, gpu, A, M, b, m, *, x0=None, rtol=NOSTOP, maxiter=1, cycle=0):
    with gpu.capture_arnoldi(cycle):
        x, info = vk.gmres(A, b, x0=x0, rtol=rtol, M=M, restart=m, maxiter=maxiter, basis="float32")
    st, bi, cap = vk.last_stats(), vk.last_basis_info(), vk.last_arnoldi(gpu)
    assert bi.used == F32 and bi.requested == F64 and st.band == 0 and st.orth == 1 and cap.band == 0
    assert cap.cycle == st.restarts - 1 and cap.n_local == A.n_local
    V = cap.V[:cap.final_cols]
    assert np.array_equal(V, V.astype(np.float32).astype(np.float64)), "a final column is not a float32 value"
    return cr.cycle_of(cap, x, st.presid), cap, st, info


def _full(cap, m):
    assert cap.cols == m and cap.breakdown == 0
    assert cap.final_cols == (m if cap.xup_tag < 0 else max(cap.xup_tag, 1)) and cap.final_cols >= m - 1


class _Case:
    """One operator on the device with its preconditioner and the reference operators."""

    def __init__(self, vk, gpu, name, prec, layout=None, mode="auto"):
        p = twin.CONFIGS[name]
        self.p, self.n, self.b = p, p.n, _rhs(p.n)
        self.A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=gpu)
        if layout:
            self.A.set_layout(layout)
        stride = vk.vlasov_line_stride(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32))
        self.close_first = []
        kind = prec[0] if prec else None
        if kind is None:
            self.M, ref = None, None
        elif kind == "bj":
            self.M, ref = vk.block_jacobi(self.A, prec[1], mode=mode), prec
        elif kind == "line":
            self.M, ref = vk.line_jacobi(self.A, stride, prec[1]), ("line", stride, prec[1])
        elif kind == "product":
            d1, d2 = (stride, prec[1]), (1, prec[2])
            self.M, ref = vk.line_product(self.A, d1, d2), ("product", d1, d2)
        elif kind == "cyclic":
            self.M, ref = vk.line_cyclic(self.A, stride, p.shape[0], prec[1]), ("cyclic", stride, p.shape[0])
        elif kind == "neumann":
            self.M_base = vk.block_jacobi(self.A, prec[1])
            self.M, ref = vk.neumann(self.A, self.M_base, prec[2]), prec
            self.close_first = [self.M]      # the wrapper borrows its base: it goes first
        self.ops = cr.Ops(self.A.download(), p.n, ref)

    def close(self):
        for m in self.close_first:
            m.close()
        M = getattr(self, "M_base", self.M)
        if M is not None:
            M.close()
        self.A.close()


RATIOS = {}


def _cycle_case(vk, gpu, c, m, tag, **tune):
    with gpu.tuning(**tune):
        cyc, cap, st, _ = _run(vk, gpu, c.A, c.M, c.b, m)
    _full(cap, m)
    cr.compare(tag, c.ops, c.b, cyc, out=RATIOS.setdefault(tag.split("|")[0], {}))
    return cap


# ---- storage --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s2(vk_lib, gpu):
    c = _Case(vk_lib, gpu, "S2", ("bj", 8))
    yield c
    c.close()


def test_storage(vk_lib, gpu, s2):
    """float32 columns, the info record, a smaller workspace, no band step.  (Fails without the
    feature: gmres has no ``basis`` argument.)"""
    vk, c = vk_lib, s2
    x64, i64 = vk.gmres(c.A, c.b, rtol=1e-8, M=c.M)
    b64, st64 = vk.last_basis_info(), vk.last_stats()
    assert i64 == 0 and b64.used == F64 and st64.band == 1
    cyc, cap, st, info = _run(vk, gpu, c.A, c.M, c.b, 20, rtol=1e-8, maxiter=400, cycle=-2)
    b32 = vk.last_basis_info()
    assert info == 0 and b32.used == F32 and st.band == 0
    assert b32.workspace_bytes < b64.workspace_bytes and b32.basis_bytes < b64.basis_bytes
    ld = -(-c.n // 64) * 64
    assert b64.basis_bytes == 21 * ld * 8 and b32.basis_bytes == 21 * ld * 4 + 2 * ld * 8
    assert cap.final_cols >= 1


# ---- the smallest shapes at which the kernels can go wrong ------------------------------------
RESTARTS = [1, 2, 8, 9, 16, 17, 24, 25, 32]


@functools.lru_cache(maxsize=None)
def _outlier(n):
    csr = cases.outlier_op(n, nout=26 if n > 64 else 0)
    return csr, cr.Ops(csr, n, None), float(np.linalg.svd(cases.dense(*csr), compute_uv=False)[-1])


@pytest.mark.parametrize("m", RESTARTS)
@pytest.mark.parametrize("n", [1025, 1, 3, 5, 1026, 1027])
def test_row_tails(vk_lib, gpu, n, m):
    vk = vk_lib
    (ip, ix, d), ops, smin = _outlier(n)
    A = vk.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu)
    b = _rhs(n)
    try:
        if m < n:
            cyc, cap, st, _ = _run(vk, gpu, A, None, b, m)
            _full(cap, m)
            cr.compare(f"tails|n={n} m={m}", ops, b, cyc, out=RATIOS.setdefault("tails", {}))
        else:   # the space is exhausted inside the cycle: the natural end, against the dense solution
            x, info = vk.gmres(A, b, rtol=1e-10, restart=m, basis="float32")
            st = vk.last_stats()
            Ad = cases.dense(ip, ix, d)
            xd = np.linalg.solve(Ad, b)
            r = np.linalg.norm(b - Ad @ x)
            assert info == 0 and vk.last_basis_info().used == F32 and r <= st.atol_eff, (info, r, st.atol_eff)
            assert np.linalg.norm(x - xd) <= (r + np.linalg.norm(b - Ad @ xd)) / smin
    finally:
        A.close()


@pytest.mark.parametrize("m", RESTARTS)
def test_several_workgroups(vk_lib, gpu, s2, m):
    _cycle_case(vk_lib, gpu, s2, m, f"S2 bj8|m={m}")


# ---- every operator-step form ---------------------------------------------------------------
FORMS = [
    ("S2", ("bj", 8), {"mode": "tridiag"}, 13), ("S2", ("bj", 8), {"mode": "inverse"}, 13),
    ("S2", ("bj", 4), {}, 13), ("S2", ("bj", 16), {}, 13), ("S2", None, {}, 13),
    ("S2", ("line", 25), {}, 8), ("S4F", ("product", 3, 5), {}, 12), ("S2", ("cyclic", 25), {}, 3),
    ("S2", ("neumann", 8, 2), {}, 12),
    ("S2", ("bj", 8), {"layout": "csr"}, 13), ("S2", ("bj", 8), {"layout": "sell"}, 13),
    ("S2", ("bj", 8), {"layout": "sell32"}, 13),
]


@pytest.mark.parametrize("name,prec,kw,m", FORMS, ids=[f"{f[0]}-{f[1]}-{f[2]}".replace(" ", "") for f in FORMS])
def test_operator_step_forms(vk_lib, gpu, name, prec, kw, m):
    c = _Case(vk_lib, gpu, name, prec, **kw)
    try:
        _cycle_case(vk_lib, gpu, c, m, f"forms|{name} {prec} {kw} m={m}")
    finally:
        c.close()


@pytest.mark.parametrize("m", [2, 20])
@pytest.mark.parametrize("tune", [{}, {"g4_ring": 0}], ids=["ring", "g4_ring0"])
@pytest.mark.parametrize("name", ["S4", "S4F"])
def test_4d_steps(vk_lib, gpu, name, tune, m):
    c = _Case(vk_lib, gpu, name, ("bj", 8))
    try:
        _cycle_case(vk_lib, gpu, c, m, f"4d|{name} {tune or 'ring'} m={m}", **tune)
    finally:
        c.close()


# ---- natural stops ----------------------------------------------------------------------------
def _natural(vk, gpu, c, name, restart, x0, rtol=1e-8):
    """A solve to its natural end against the restatement and against SciPy's solve."""
    ip, ix, d = c.ops.f64.indptr, c.ops.f64.indices, c.ops.f64.data
    As = twin.scipy_csr(ip, ix, d, c.n)
    ref = cr.solve_cb(c.ops.f64, c.b, x0, rtol=rtol, restart=restart)
    tab = cr.solve_cb(c.ops.f64, c.b, x0, rtol=rtol, restart=restart, schedule="fixed")   # the iteration table's schedule
    x, info = vk.gmres(c.A, c.b, x0=x0, rtol=rtol, M=c.M, restart=restart, basis="float32")
    st, bi = vk.last_stats(), vk.last_basis_info()
    r = float(np.linalg.norm(c.b - As @ x))
    print(f"CBN|{name} restart={restart} x0={'0' if x0 is None else 'set'}|device {st.inner_iters} in {st.restarts} cycles, "
          f"|r| {r:.3e}|restatement {ref.inner_iters} in {ref.cycles} (fixed ptol: {tab.inner_iters} in {tab.cycles})|atol {st.atol_eff:.3e}")
    assert info == 0 == ref.info and bi.used == F32 and st.band == 0
    assert r <= st.atol_eff
    assert abs(st.inner_iters - ref.inner_iters) <= 1, (st.inner_iters, ref.inner_iters)
    assert tab.info == 0 and abs(st.inner_iters - tab.inner_iters) <= 1, (st.inner_iters, tab.inner_iters)
    from scipy.sparse.linalg import LinearOperator, gmres
    Ms = LinearOperator((c.n, c.n), matvec=lambda v: c.ops.f64.Minv(np.asarray(v).reshape(-1)), dtype=np.float64)
    xs, infos = gmres(As, c.b, x0=x0, rtol=rtol, restart=restart, M=Ms)
    rs = float(np.linalg.norm(c.b - As @ xs))
    assert infos == 0
    assert np.linalg.norm(x - xs) <= (r + rs) / _sigma_min(name), (np.linalg.norm(x - xs), r, rs)
    return st, ref


@pytest.mark.parametrize("x0set", [False, True], ids=["x0=0", "x0"])
@pytest.mark.parametrize("restart", [20, 5])
def test_natural_stop_s2(vk_lib, gpu, s2, restart, x0set):
    """restart 20: 68 = 3 * 20 + 8, the x update inside an update pass; restart 5: cycles that end
    at the closing reduction (the host-enqueued x update) and one that stops inside."""
    x0 = twin.rhs(s2.n, seed=0xB00) * 1e-3 if x0set else None
    _natural(vk_lib, gpu, s2, "S2", restart, x0)


@pytest.mark.parametrize("restart", [20, 5])
def test_natural_stop_s4f(vk_lib, gpu, restart):
    c = _Case(vk_lib, gpu, "S4F", ("bj", 8))
    try:
        _natural(vk_lib, gpu, c, "S4F", restart, None)
    finally:
        c.close()


def test_natural_stop_xline_extra_cycle(vk_lib, gpu):
    """S2 with the x-line preconditioner at restart 20: the float64 basis needs 12 iterations in one
    cycle, and that cycle reduces the residual by more than a float32 basis can carry: the extra
    cycle must appear -- two cycles, 13 +- 1 iterations."""
    c = _Case(vk_lib, gpu, "S2", ("line", 25))
    try:
        x, info = vk_lib.gmres(c.A, c.b, rtol=1e-8, M=c.M, restart=20, basis="float64")
        s64 = vk_lib.last_stats()
        assert info == 0 and s64.inner_iters == 12 and s64.restarts == 1
        st, ref = _natural(vk_lib, gpu, c, "S2", 20, None)
        assert st.restarts == 2 and ref.cycles == 2
        assert abs(st.inner_iters - 13) <= 1, st.inner_iters
    finally:
        c.close()


# ---- no leak ----------------------------------------------------------------------------------
def test_no_leak(vk_lib, gpu, s2):
    """float64, float32, float64 on one context: the third solve is the first, bit for bit."""
    vk, c = vk_lib, s2

    def solve(basis):
        x, info = vk.gmres(c.A, c.b, rtol=1e-8, M=c.M, basis=basis)
        st = vk.last_stats()
        return x, info, {k: v for k, v in vars(st).items() if k != "t_solve"}, vk.last_basis_info()
    x1, i1, s1, b1 = solve(None)
    x2, i2, s2_, b2 = solve("float32")
    x3, i3, s3, b3 = solve(None)
    assert b1.used == F64 and b2.used == F32 and b3.used == F64 and gpu.basis == F64
    assert s2_["band"] == 0 and s1["band"] == 1 and s3["band"] == 1
    assert i1 == i3 == 0 and np.array_equal(x1, x3) and s1 == s3 and b1 == b3


# ---- refusals -----------------------------------------------------------------------------------
def test_refusals(vk_lib, gpu, s2):
    vk, c = vk_lib, s2
    with pytest.raises(ValueError, match="DCGS2"):
        vk.gmres(c.A, c.b, rtol=1e-8, M=c.M, orth="mgs", basis="float32")
    with pytest.raises(ValueError, match="DCGS2"):
        vk.gmres(c.A, c.b, rtol=1e-8, M=c.M, restart=33, basis="float32")
    with pytest.raises(ValueError):
        vk.gmres(c.A, c.b, rtol=1e-8, M=c.M, restart=33, orth="dcgs2", basis="float32")
    for bad in (2, -1, 7):
        assert vk._abi.lib().vtk_gmres_set_basis(gpu.handle, bad) == vk._abi.ERR_ARG
    with pytest.raises(ValueError):
        gpu.set_basis(5)
    with pytest.raises(ValueError):
        vk.gmres(c.A, c.b, M=c.M, basis="float16")
    assert gpu.basis == F64 and gpu.basis_info().requested == F64
    x, info = vk.gmres(c.A, c.b, rtol=1e-8, M=c.M)      # the context still solves, with the band
    assert info == 0 and vk.last_stats().band == 1


# ---- across ranks (host-staged communicator, ranks sharing the GPU) -----------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, case, mixed, outdir):
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
    out = {}
    if mixed:   # the ranks disagree: every rank is refused, and the communicator still works
        try:
            vk.gmres(A, b, rtol=1e-8, M=M, basis="float32" if rank == 0 else "float64")
            out["refused"] = ""
        except ValueError as e:
            out["refused"] = str(e)
        x, info = vk.gmres(A, b, rtol=1e-8, M=M, basis="float32")
        out.update(x=x, info=info, iters=vk.last_stats().inner_iters, used=vk.last_basis_info().used)
    else:
        x, info = vk.gmres(A, b, rtol=1e-8, M=M, basis="float32")
        st = vk.last_stats()
        out.update(x=x, info=info, iters=st.inner_iters, used=vk.last_basis_info().used, band=st.band,
                   cycles=st.restarts)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), commlog=json.dumps(hc.log), **out)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(tmp_path, case, world, mixed):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), case, mixed, str(tmp_path)), nprocs=world, join=True)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    for q in z:
        assert q["errors"].size == 0, q["errors"]
    from vtkrylov.comm import check_sequences
    check_sequences([json.loads(str(q["commlog"])) for q in z])
    return z


@pytest.mark.parametrize("case,world", [("S2", 2), ("S2", 3), ("S4", 2), ("S4", 3)])
def test_across_ranks(vk_lib, gpu, tmp_path, case, world):
    z = _spawn(tmp_path, case, world, False)
    c = _Case(vk_lib, gpu, case, ("bj", 8))
    try:
        x1, info1 = vk_lib.gmres(c.A, c.b, rtol=1e-8, M=c.M, basis="float32")
        st1 = vk_lib.last_stats()
        As = twin.scipy_csr(c.ops.f64.indptr, c.ops.f64.indices, c.ops.f64.data, c.n)
        x = np.concatenate([q["x"] for q in z])
        r, r1 = float(np.linalg.norm(c.b - As @ x)), float(np.linalg.norm(c.b - As @ x1))
        for q in z:
            assert int(q["info"]) == info1 == 0 and int(q["used"]) == F32 and int(q["band"]) == 0
            assert int(q["iters"]) == int(z[0]["iters"]) and abs(int(q["iters"]) - st1.inner_iters) <= 1
        assert r <= st1.atol_eff
        assert np.linalg.norm(x - x1) <= (r + r1) / _sigma_min(case)
    finally:
        c.close()


def test_ranks_disagree(tmp_path):
    z = _spawn(tmp_path, "S2", 2, True)
    for q in z:
        assert "disagree" in str(q["refused"]), str(q["refused"])
        assert int(q["info"]) == 0 and int(q["used"]) == F32
