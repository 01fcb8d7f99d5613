"""vtkrylov.bicgstab on the GPU against the NumPy twin of scipy.sparse.linalg.bicgstab
(tests/test_bicgstab_host.py pins the twin to SciPy bit for bit).  The operator is the oracle
generator's, the right-hand side twin.rhs; the twin's preconditioner is the oracle's block-Jacobi
inverse / line factors (the GPU setup's bits).

Bars of the parity grid: info equal and 0; ||b - A x|| recomputed on the host <= 1.01 atol_eff (the
exit test is on the recurrence residual; its drift from the true one is of order iterations eps
||A|| ||x||, five orders under 1 % of atol at rtol 1e-8); |iterations - ref| <= max(2, ceil(0.15
ref)); ||x - x_ref|| <= 4 rtol ||x_ref||.  The last two come from running the twin on the CPU with
three summation orders of its dots (np.dot, 509 strided partials summed in reverse, a running sum)
on S2, S4, C0, C1 x {none, BJ(8), line} x rtol 1e-5 / 1e-8 / 1e-11: worst iteration shift 8.8 %
(62 vs 57, no preconditioner), 5.8 % with BJ, 0 with line; worst x difference 0.94 rtol at rtol
1e-5 and 1e-8, 1.4 rtol at 1e-11; true residual / atol_eff 1.000.  Both iterates satisfy the same
residual bound, so 2 atol ||A^-1|| limits their difference; rounding does not.  With the line
preconditioner the summation order moved x by at most 7e-13 relative and never moved the count:
those cases are held to equal counts and the project's 1e-9 bar.

Every solve passes maxiter <= 500: a stop-logic defect ends in a failed assertion, not in a
10 n-iteration loop.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest

from oracle import coracle, twin
from test_bicgstab_host import BREAKDOWNS, bicgstab_twin, general_csr

pytestmark = pytest.mark.gpu

MAXIT = 500
P1 = dict(cfl=8.0, E0=0.8, nu=0.1)   # tests/test_gpu_update.py's second set of values


def cfg(name, which=0):
    p = twin.CONFIGS[name]
    return dataclasses.replace(p, **P1) if which else p


@functools.lru_cache(maxsize=None)
def gen(name, which=0):
    out = coracle.generate(cfg(name, which))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_matrix(name, which=0):
    ip, ix, d = gen(name, which)
    return twin.scipy_csr(ip, ix, d.astype(np.float64), cfg(name).n)


def line_geometry(name):
    p = cfg(name)
    if p.dim == 1:
        return 1, 25
    if p.dim == 2:
        return p.shape[1], 25
    return p.shape[1] * p.shape[2] * p.shape[3], 3


@functools.lru_cache(maxsize=None)
def host_prec(name, kind, which=0):
    """The twin's M as a callable: None, the oracle's BJ inverse rows or its line factors."""
    ip, ix, d = gen(name, which)
    if kind == "none":
        return None
    if kind.startswith("bj"):
        inv = coracle.bj_setup(ip, ix, d, int(kind[2:]))
        return lambda r: coracle.bj_apply(inv, np.ascontiguousarray(r))
    lf = coracle.line_setup(ip, ix, d, *line_geometry(name))
    return lambda r: coracle.line_apply(lf, np.ascontiguousarray(r))


@functools.lru_cache(maxsize=None)
def ref(name, kind, rtol, maxiter=MAXIT, x0_seed=None):
    """(x, info, iterations, half_step) of the twin; computed once, never written to."""
    n = cfg(name).n
    x0 = None if x0_seed is None else twin.rhs(n, seed=x0_seed)
    out = bicgstab_twin(host_matrix(name), twin.rhs(n), x0, rtol=rtol, maxiter=maxiter, M=host_prec(name, kind))
    out[0].setflags(write=False)
    return out


def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


def operator(vk, gpu, name, layout=None, which=0):
    A = vk.vlasov_operator(vparams(vk, cfg(name, which)), ctx=gpu)
    if layout:
        A.set_layout(layout)
    return A


def device_prec(vk, A, name, kind, mode="auto"):
    if kind == "none":
        return None
    if kind.startswith("bj"):
        return vk.block_jacobi(A, int(kind[2:]), mode)
    return vk.line_jacobi(A, *line_geometry(name))


def true_residual(csr, b, x):
    ip, ix, d = csr
    return np.linalg.norm(b - coracle.spmv(ip, ix, d, np.ascontiguousarray(x)))


def within_bars(x, info, st, r, csr, b, rtol):
    xr, infor, itr, halfr = r
    print(f"info {info} (ref {infor}) iterations {st.iterations} (ref {itr}) half {st.half_step} (ref {halfr})")
    assert info == infor == 0
    res = true_residual(csr, b, x)
    atol_eff = rtol * np.linalg.norm(b)
    print(f"true residual / atol_eff {res / atol_eff:.6f}")
    assert res <= 1.01 * atol_eff, (res, atol_eff)
    assert abs(st.iterations - itr) <= max(2, math.ceil(0.15 * itr)), (st.iterations, itr)
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    print(f"x difference / rtol {rel / rtol:.3f}")
    assert rel <= 4 * rtol, rel


# ---- 1. parity grid ---------------------------------------------------------------------------

GRID = [(name, kind, mode) for name in ("S2", "S4", "S4F", "C0")
        for kind, mode in (("none", "auto"), ("bj8", "auto"), ("bj8", "inverse"), ("bj16", "auto"), ("line", "auto"))]
GRID += [("C1", "bj8", "auto"), ("C1", "line", "auto")]


@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
@pytest.mark.parametrize("layout", ["csr", "sell"])
@pytest.mark.parametrize("name,kind,mode", GRID)
def test_parity_grid(vk_lib, gpu, name, kind, mode, layout, rtol):
    A = operator(vk_lib, gpu, name, layout)
    M = device_prec(vk_lib, A, name, kind, mode)
    b = twin.rhs(cfg(name).n)
    x, info = vk_lib.bicgstab(A, b, rtol=rtol, M=M, maxiter=MAXIT)
    st = vk_lib.last_bicgstab_stats()
    within_bars(x, info, st, ref(name, kind, rtol), gen(name), b, rtol)
    # the reported residual is the true one of the returned x
    assert abs(st.rnorm - true_residual(gen(name), b, x)) <= 1e-6 * st.atol_eff
    assert st.bnorm == pytest.approx(np.linalg.norm(b), rel=1e-12) and st.atol_eff == rtol * st.bnorm
    for o in (M, A):
        if o is not None:
            o.close()


# ---- 2. the line-preconditioned cases are sharp ------------------------------------------------

@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
@pytest.mark.parametrize("name", ["S2", "C0", "C1"])
def test_line_cases_are_sharp(vk_lib, gpu, name, rtol):
    xr, infor, itr, halfr = ref(name, "line", rtol)
    if rtol == 1e-8 and name == "S2":
        assert (itr, halfr) == (8, 1)     # leaves through the half step
    if rtol == 1e-8 and name == "C1":
        assert (itr, halfr) == (8, 0)     # leaves at the top
    A = operator(vk_lib, gpu, name)
    M = device_prec(vk_lib, A, name, "line")
    x, info = vk_lib.bicgstab(A, twin.rhs(cfg(name).n), rtol=rtol, M=M, maxiter=MAXIT)
    st = vk_lib.last_bicgstab_stats()
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    print(f"iterations {st.iterations} (ref {itr}) half {st.half_step} (ref {halfr}) x_rel {rel:.3e}")
    assert info == infor == 0
    assert st.iterations == itr and st.half_step == halfr
    assert rel <= 1e-9, rel
    M.close()
    A.close()


# ---- 3. truncated run ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "S4F"])
def test_truncated_run(vk_lib, gpu, name):
    xr, infor, itr, _ = ref(name, "bj8", 1e-8, maxiter=3)
    assert infor == 3 and itr == 3
    A = operator(vk_lib, gpu, name)
    M = vk_lib.block_jacobi(A, 8)
    x, info = vk_lib.bicgstab(A, twin.rhs(cfg(name).n), rtol=1e-8, M=M, maxiter=3)
    st = vk_lib.last_bicgstab_stats()
    assert info == 3 and st.iterations == 3 and st.half_step == 0
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    assert rel <= 1e-9, rel
    M.close()
    A.close()


# ---- 4, 5, 6. b = 0, an exact x0, a non-zero x0 -------------------------------------------------

def test_zero_b(vk_lib, gpu):
    n = cfg("S2").n
    A = operator(vk_lib, gpu, "S2")
    x, info = vk_lib.bicgstab(A, np.zeros(n), twin.rhs(n, seed=3), rtol=1e-8, maxiter=MAXIT)
    assert info == 0 and vk_lib.last_bicgstab_stats().iterations == 0
    assert x.shape == (n,) and not x.any()
    A.close()


def test_exact_x0(vk_lib, gpu):
    n = cfg("S2").n
    b = twin.rhs(n)
    x0 = bicgstab_twin(host_matrix("S2"), b, rtol=1e-12, maxiter=MAXIT, M=host_prec("S2", "bj8"))[0]
    assert true_residual(gen("S2"), b, x0) < 1e-9 * np.linalg.norm(b)
    A = operator(vk_lib, gpu, "S2")
    M = vk_lib.block_jacobi(A, 8)
    x, info = vk_lib.bicgstab(A, b, x0, rtol=1e-8, M=M, maxiter=MAXIT)
    st = vk_lib.last_bicgstab_stats()
    assert info == 0 and st.iterations == 0 and st.half_step == 0
    assert np.array_equal(x, x0)
    M.close()
    A.close()


def test_nonzero_x0_host_and_device(vk_lib, gpu):
    import torch
    n = cfg("S2").n
    b, x0 = twin.rhs(n), twin.rhs(n, seed=3)
    A = operator(vk_lib, gpu, "S2")
    M = vk_lib.block_jacobi(A, 8)
    x, info = vk_lib.bicgstab(A, b, x0, rtol=1e-8, M=M, maxiter=MAXIT)
    st = vk_lib.last_bicgstab_stats()
    within_bars(x, info, st, ref("S2", "bj8", 1e-8, x0_seed=3), gen("S2"), b, 1e-8)
    assert np.array_equal(x0, twin.rhs(n, seed=3))   # x0 is not written
    dev = torch.device("cuda", gpu.device)
    tb, tx0 = torch.from_numpy(b).to(dev), torch.from_numpy(x0).to(dev)
    tx, tinfo = vk_lib.bicgstab(A, tb, tx0, rtol=1e-8, M=M, maxiter=MAXIT)
    assert isinstance(tx, torch.Tensor) and tx.is_cuda and tinfo == info
    assert vk_lib.last_bicgstab_stats().iterations == st.iterations
    assert np.array_equal(tx.cpu().numpy(), x)       # the same kernels on the same bits
    assert np.array_equal(tx0.cpu().numpy(), x0)
    M.close()
    A.close()


# ---- 7. exact breakdowns ------------------------------------------------------------------------

@pytest.mark.parametrize("copies", [1, 64])
@pytest.mark.parametrize("case", range(len(BREAKDOWNS)))
def test_exact_breakdowns(vk_lib, gpu, case, copies):
    import scipy.sparse as sp
    A3, b3, (want_info, want_its) = BREAKDOWNS[case]
    H = sp.kron(sp.identity(copies), sp.csr_matrix(np.array(A3, dtype=np.float64)), format="csr")
    b = np.tile(np.array(b3, dtype=np.float64), copies)
    xr, infor, itr, _ = bicgstab_twin(H, b, rtol=1e-12, maxiter=MAXIT)
    assert (infor, itr) == (want_info, want_its)
    A = vk_lib.csr_matrix(H, ctx=gpu)
    x, info = vk_lib.bicgstab(A, b, rtol=1e-12, maxiter=MAXIT)
    st = vk_lib.last_bicgstab_stats()
    assert (info, st.iterations, st.half_step) == (want_info, want_its, 0)
    if want_its == 0:
        assert not x.any()
    assert np.array_equal(x, xr)   # every intermediate is dyadic: the same bits in any summation order
    A.close()


# ---- 8. general CSR -----------------------------------------------------------------------------

@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
@pytest.mark.parametrize("kind", ["none", "bj8"])
def test_general_csr(vk_lib, gpu, kind, rtol):
    R = general_csr()
    n = R.shape[0]
    csr = (R.indptr.astype(np.int32), R.indices.astype(np.int32), R.data)
    b = twin.rhs(n)
    Mh = None
    if kind == "bj8":
        inv = coracle.bj_setup(*csr, 8)
        Mh = lambda r: coracle.bj_apply(inv, np.ascontiguousarray(r))
    r = bicgstab_twin(R, b, rtol=rtol, maxiter=MAXIT, M=Mh)
    A = vk_lib.csr_matrix(R, ctx=gpu)
    M = vk_lib.block_jacobi(A, 8) if kind == "bj8" else None
    x, info = vk_lib.bicgstab(A, b, rtol=rtol, M=M, maxiter=MAXIT)
    within_bars(x, info, vk_lib.last_bicgstab_stats(), r, csr, b, rtol)
    for o in (M, A):
        if o is not None:
            o.close()


# ---- 9. determinism and the fused pin -----------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "S4F"])
def test_two_solves_are_bit_identical(vk_lib, gpu, name):
    A = operator(vk_lib, gpu, name)
    M = vk_lib.block_jacobi(A, 8)
    b = twin.rhs(cfg(name).n)
    x1, i1 = vk_lib.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    s1 = vk_lib.last_bicgstab_stats()
    x2, i2 = vk_lib.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    s2 = vk_lib.last_bicgstab_stats()
    assert i1 == i2 == 0 and s1.iterations == s2.iterations and s1.half_step == s2.half_step
    assert np.array_equal(x1, x2)
    M.close()
    A.close()


@pytest.mark.parametrize("name,bs,mode", [("S2", 8, "tridiag"), ("S2", 8, "inverse"), ("S2", 4, "auto"),
                                          ("S4F", 8, "tridiag"), ("S4F", 8, "inverse"), ("S4F", 4, "auto")])
def test_fused_forms_are_bit_identical(vk_lib, gpu, name, bs, mode):
    """bcg_fuse 1 (phat = M p, shat = M s inside k_bcg_p / k_bcg_s) against the separate apply."""
    A = operator(vk_lib, gpu, name)
    M = vk_lib.block_jacobi(A, bs, mode)
    if mode != "auto":
        assert M.mode == mode
    b = twin.rhs(cfg(name).n)
    assert gpu.get_tuning("bcg_fuse") == 1
    x1, i1 = vk_lib.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    s1 = vk_lib.last_bicgstab_stats()
    with gpu.tuning(bcg_fuse=0):
        x0, i0 = vk_lib.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
        s0 = vk_lib.last_bicgstab_stats()
    assert gpu.get_tuning("bcg_fuse") == 1
    assert i1 == i0 == 0 and (s1.iterations, s1.half_step) == (s0.iterations, s0.half_step)
    assert np.array_equal(x1, x0)
    M.close()
    A.close()


# ---- 10. preconditioner state -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "S4F"])
def test_lagged_preconditioner_still_solves(vk_lib, gpu, name):
    p1 = cfg(name, 1)
    A = operator(vk_lib, gpu, name)
    M = vk_lib.block_jacobi(A, 8)
    A.update_vlasov(vparams(vk_lib, p1))
    assert (A.values_epoch, M.values_epoch) == (1, 0)
    b = twin.rhs(p1.n)
    x, info = vk_lib.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    assert info == 0
    res = true_residual(gen(name, 1), b, x)
    assert res <= 1.01 * 1e-8 * np.linalg.norm(b), res
    M.close()
    A.close()


def test_failed_refresh_is_refused(vk_lib, gpu):
    ip, ix, d1 = gen("S2", 1)
    dz = d1.copy()
    dz[ip[40]:ip[48]] = 0.0   # every entry of the rows of 8-block 5
    A = operator(vk_lib, gpu, "S2")
    M = vk_lib.block_jacobi(A, 8)
    L = vk_lib.line_jacobi(A, cfg("S2").shape[1], 16)
    A.update_values(dz)
    for P in (M, L):
        with pytest.raises(np.linalg.LinAlgError):
            P.refresh()
        with pytest.raises(vk_lib._abi.VtkError) as e:
            vk_lib.bicgstab(A, twin.rhs(cfg("S2").n), M=P, maxiter=MAXIT)
        assert e.value.status == vk_lib._abi.ERR_STATE
    for o in (L, M, A):
        o.close()


# ---- 11. entry layer ----------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["block_jacobi", "line_jacobi"])
def test_entry_layer_runs_bicgstab(vk_lib, gpu, tmp_path, prec):
    from vtsetup.config import SolverConfig
    from vtsetup.krylov_precondition import KrylovPrecondition
    c = SolverConfig.load(config="S2", method="bicgstab", preconditioner=prec, report=str(tmp_path / "report.json"))
    c.maxiter = MAXIT
    step = KrylovPrecondition(c, ctx=gpu)
    res = step.main()
    st = vk_lib.last_bicgstab_stats()
    s = res["solve"]
    assert s["method"] == "bicgstab" and s["info"] == 0
    assert s["iterations"] == st.iterations and s["half_step"] == st.half_step
    assert set(s) >= {"method", "info", "iterations", "half_step", "rnorm", "bnorm", "t_solve_s"}
    b = vk_lib.rhs_splitmix(c.shape[0] * c.shape[1], seed=c.seed)
    assert true_residual(gen("S2"), b, np.asarray(step.x)) <= 1.01 * c.rtol * np.linalg.norm(b)
