"""Value updates and preconditioner refreshes: an operator whose sparsity pattern
stays and whose values change every time step.  The rule under test: after ``update_values`` /
``update_vlasov`` the operator is indistinguishable from one freshly created with those values,
and a refreshed preconditioner from a freshly created one -- downloads, SpMV bits in every
layout, line values / 4D grid tables (lost and regained with the values), the factors, and the
solves, bit for bit.  A preconditioner that was not refreshed keeps its old factors and still
solves (a lagged preconditioner).

p0 = a config's default parameters, p1 = cfl 8, E0 0.8, nu 0.1: the same pattern, other values.
"""
import dataclasses
import functools
import json
import os
import socket

import numpy as np
import pytest

from oracle import coracle, twin

pytestmark = pytest.mark.gpu

P1 = dict(cfl=8.0, E0=0.8, nu=0.1)
SHAPES = dict(twin.CONFIGS, V7=twin.Vlasov(2, (7, 24)))   # V7: n = 168, no multiple of 64, 7 lines


def cfg(name, which):
    p = SHAPES[name]
    return dataclasses.replace(p, **P1) if which else p


@functools.lru_cache(maxsize=None)
def gen(name, which):
    """(indptr, indices, data) of the oracle generator; shared by the tests, never written to."""
    out = coracle.generate(cfg(name, which))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_solve(name, which_a, which_m, kind="bj"):
    """coracle.gmres on the `which_a` values with the preconditioner from the `which_m` values."""
    ip, ix, d = gen(name, which_a)
    mp, mx, md = gen(name, which_m)
    p = cfg(name, which_a)
    pre = coracle.bj_setup(mp, mx, md, 8) if kind == "bj" else coracle.line_setup(mp, mx, md, p.shape[1], 16)
    return coracle.gmres(ip, ix, d, twin.rhs(p.n), pre, rtol=1e-8)


def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


def fresh(vk, gpu, name, which):
    return vk.vlasov_operator(vparams(vk, cfg(name, which)), ctx=gpu)


def solve(vk, A, M, b):
    x, info = vk.gmres(A, b, rtol=1e-8, M=M)
    return x, info, vk.last_stats()


def same_operator(A, F, x):
    """A is indistinguishable from F: download, SpMV bits, tables, layout."""
    for a, f in zip(A.download(), F.download()):
        assert a.dtype == f.dtype and np.array_equal(a.view(np.uint8), f.view(np.uint8))
    assert np.array_equal(A @ x, F @ x)
    assert (A.line_band, A.line_values, A.grid4) == (F.line_band, F.line_values, F.grid4)
    assert A.layout_info() == F.layout_info()


def within_bars(x, info, st, ref):
    assert info == ref.info == 0
    assert abs(st.inner_iters - ref.inner_iters) <= 1, (st.inner_iters, ref.inner_iters)
    rel = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
    assert rel <= 1e-9, rel


# ---- 1. update equals fresh ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "V7", "S4", "S4F", "C0"])
def test_update_vlasov_equals_fresh(vk_lib, gpu, name):
    p1 = cfg(name, 1)
    ip, ix, d1 = gen(name, 1)
    assert np.array_equal(gen(name, 0)[1], ix) and not np.array_equal(gen(name, 0)[2], d1)
    A = fresh(vk_lib, gpu, name, 0)
    assert A.values_epoch == 0
    assert A.update_vlasov(vparams(vk_lib, p1)) is A
    assert A.values_epoch == 1
    F = fresh(vk_lib, gpu, name, 1)
    x = twin.rhs(p1.n, seed=0xC0FFEE)
    same_operator(A, F, x)
    gip, gix, gd = A.download()
    assert np.array_equal(gip, ip) and np.array_equal(gix, ix)
    assert gd.dtype == d1.dtype and np.array_equal(gd.view(np.uint8), d1.view(np.uint8))
    assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1, x))
    if p1.dim == 2:
        assert A.line_band == p1.shape[1] and A.line_values == 2
    if p1.dim == 4:
        assert A.grid4 == tuple(p1.shape[1:])
    # another shape, dim or value type is no update of this operator; a CSR upload has no parameters
    other = dataclasses.replace(p1, shape=tuple(reversed(p1.shape)) if p1.dim == 2 else p1.shape, fp32=not p1.fp32)
    with pytest.raises(ValueError):
        A.update_vlasov(vparams(vk_lib, other))
    assert A.values_epoch == 1 and np.array_equal(A @ x, F @ x)
    U = vk_lib.csr_matrix((d1, ix, ip), shape=(p1.n, p1.n), ctx=gpu)
    with pytest.raises(vk_lib._abi.VtkError) as e:
        U.update_vlasov(vparams(vk_lib, p1))
    assert e.value.status == vk_lib._abi.ERR_STATE
    for o in (U, F, A):
        o.close()


@pytest.mark.parametrize("how", ["host", "device"])
@pytest.mark.parametrize("name", ["S2", "V7", "S4", "S4F", "C0"])
def test_update_values_equals_fresh(vk_lib, gpu, name, how):
    p = cfg(name, 1)
    ip, ix, d0 = gen(name, 0)
    d1 = gen(name, 1)[2]
    assert d1.dtype == (np.float32 if p.fp32 else np.float64)
    # the generated operator and the uploaded CSR both take new values
    for A in (fresh(vk_lib, gpu, name, 0), vk_lib.csr_matrix((d0, ix, ip), shape=(p.n, p.n), ctx=gpu)):
        if how == "device":
            import torch
            A.update_values(torch.from_numpy(d1.copy()).to(torch.device("cuda", gpu.device)))
        else:
            A.update_values(d1)
        assert A.values_epoch == 1
        F = vk_lib.csr_matrix((d1, ix, ip), shape=(p.n, p.n), ctx=gpu)
        x = twin.rhs(p.n, seed=0xC0FFEE)
        same_operator(A, F, x)
        assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1, x))
        F.close()
        A.close()


@pytest.mark.parametrize("layout", ["csr", "sell", "sell32"])
@pytest.mark.parametrize("name", ["S2", "V7", "S4F", "C0"])
def test_update_in_every_layout(vk_lib, gpu, name, layout):
    p1 = cfg(name, 1)
    ip, ix, d1 = gen(name, 1)
    A = fresh(vk_lib, gpu, name, 0)
    A.set_layout(layout)
    A.update_vlasov(vparams(vk_lib, p1))
    F = fresh(vk_lib, gpu, name, 1)
    F.set_layout(layout)
    x = twin.rhs(p1.n, seed=0xC0FFEE)
    assert A.layout == F.layout == layout
    same_operator(A, F, x)
    assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1, x))
    # and the values arrive in a layout chosen after the update as well
    for other in ("sell", "csr", "sell32"):
        A.set_layout(other)
        assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1, x)), other
    F.close()
    A.close()


@functools.lru_cache(maxsize=None)
def ragged():
    """test_gpu_dropin.py's ragged random CSR: n = 2000, one empty row, one 600-entry row (a SELL
    chunk whose span exceeds the refresh kernel's LDS stage)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(7)
    n = 2000
    R = sp.random(n, n, density=0.003, random_state=11, format="csr") + sp.identity(n, format="csr")
    R = R.tolil()
    R[5, :] = 0
    R[17, rng.choice(n, 600, replace=False)] = 1.5
    return R.tocsr()


@pytest.mark.parametrize("layout", ["csr", "sell", "sell32"])
def test_ragged_update_in_every_layout(vk_lib, gpu, layout):
    R = ragged()
    n = R.shape[0]
    assert R.indptr[6] == R.indptr[5] and R.indptr[18] - R.indptr[17] >= 600
    A = vk_lib.csr_matrix(R, ctx=gpu)
    A.set_layout(layout)
    rng = np.random.default_rng(23)
    x = rng.standard_normal(n)
    for step in range(2):
        R2 = R.copy()
        R2.data = rng.standard_normal(R.nnz)
        A.update_values(R2.data)
        assert A.values_epoch == step + 1 and A.layout == layout
        assert np.array_equal(A @ x, R2 @ x)
        F = vk_lib.csr_matrix(R2, ctx=gpu)
        F.set_layout(layout)
        assert A.layout_info() == F.layout_info()
        F.close()
    A.close()


def test_wrong_dtype_or_length_changes_nothing(vk_lib, gpu):
    import torch
    ip, ix, d0 = gen("S2", 0)
    d1 = gen("S2", 1)[2]
    A = fresh(vk_lib, gpu, "S2", 0)
    F = fresh(vk_lib, gpu, "S4F", 0)
    x = twin.rhs(A.n_local, seed=0xC0FFEE)
    y0 = A @ x
    dev = torch.device("cuda", gpu.device)
    bad = [d1.astype(np.float32), d1[:-1], np.concatenate([d1, d1[:1]]), d1.reshape(2, -1), d1.astype(np.int64),
           torch.from_numpy(d1.astype(np.float32)).to(dev), torch.from_numpy(d1[:-1].copy()).to(dev)]
    for v in bad:
        with pytest.raises(ValueError):
            A.update_values(v)
    with pytest.raises(ValueError):   # an fp32 operator takes float32 only
        F.update_values(gen("S4F", 1)[2].astype(np.float64))
    assert A.values_epoch == 0 and F.values_epoch == 0
    assert np.array_equal(A @ x, y0) and np.array_equal(y0, coracle.spmv(ip, ix, d0, x))
    F.close()
    A.close()


# ---- 2. refresh equals fresh --------------------------------------------------------------

@pytest.mark.parametrize("name,bs,mode", [("S2", 8, "inverse"), ("S2", 8, "tridiag"), ("S2", 8, "auto"),
                                          ("V7", 8, "tridiag"), ("S4", 8, "auto"), ("S2", 5, "auto"),
                                          ("V7", 5, "auto"), ("S4F", 4, "tridiag")])
def test_bj_refresh_equals_fresh(vk_lib, gpu, name, bs, mode):
    p1 = cfg(name, 1)
    ip, ix, d1 = gen(name, 1)
    A = fresh(vk_lib, gpu, name, 0)
    M = vk_lib.block_jacobi(A, bs, mode)
    assert M.values_epoch == 0
    inv0 = M.inverse()
    A.update_vlasov(vparams(vk_lib, p1))
    assert M.values_epoch == 0 and np.array_equal(M.inverse(), inv0)   # stale until refreshed
    assert M.refresh() is M
    assert M.values_epoch == A.values_epoch == 1
    F = fresh(vk_lib, gpu, name, 1)
    MF = vk_lib.block_jacobi(F, bs, mode)
    inv = M.inverse()
    assert np.array_equal(inv, MF.inverse())
    assert np.array_equal(inv, coracle.bj_setup(ip, ix, d1, bs))   # the exact setup's bit identity
    assert M.mode == MF.mode and M.tridiag_available == MF.tridiag_available
    if mode != "auto":
        assert M.mode == mode   # the request is kept
    r = twin.rhs(p1.n, seed=5)
    assert np.array_equal(M @ r, MF @ r)
    for o in (MF, M, F, A):
        o.close()


def test_bj_mfma_refresh_equals_fresh(vk_lib, gpu):
    p1 = cfg("S2", 1)
    A = fresh(vk_lib, gpu, "S2", 0)
    M = vk_lib.block_jacobi(A, 16, setup="mfma")
    A.update_vlasov(vparams(vk_lib, p1))
    M.refresh()
    F = fresh(vk_lib, gpu, "S2", 1)
    MF = vk_lib.block_jacobi(F, 16, setup="mfma")
    assert np.array_equal(M.inverse(), MF.inverse())   # the remembered setup, bit for bit
    r = twin.rhs(p1.n, seed=5)
    assert np.array_equal(M @ r, MF @ r)
    for o in (MF, M, F, A):
        o.close()


def test_line_refresh_equals_fresh(vk_lib, gpu):
    p1 = cfg("S2", 1)
    ip, ix, d1 = gen("S2", 1)
    A = fresh(vk_lib, gpu, "S2", 0)
    L = vk_lib.line_jacobi(A, p1.shape[1], 16)
    K = vk_lib.line_jacobi(A, p1.shape[1], 16)
    K.set_compact(False)
    assert L.compact and not K.compact
    A.update_vlasov(vparams(vk_lib, p1))
    assert L.refresh() is L and L.values_epoch == 1
    K.refresh()
    F = fresh(vk_lib, gpu, "S2", 1)
    LF = vk_lib.line_jacobi(F, p1.shape[1], 16)
    f = L.factors()
    assert np.array_equal(f, LF.factors()) and np.array_equal(f, K.factors())
    assert np.array_equal(f, coracle.line_setup(ip, ix, d1, p1.shape[1], 16).f)
    assert L.compact == LF.compact is True and L.compact_available == LF.compact_available
    assert not K.compact and K.compact_available   # set_compact(False) is kept
    r = twin.rhs(p1.n, seed=5)
    z = LF @ r
    assert np.array_equal(L @ r, z) and np.array_equal(K @ r, z)
    # values whose x couplings vary along a line: the compact tables go, and come back
    d1x = d1.copy()
    d1x[ip[167]] *= 1.0625
    A.update_values(d1x)
    L.refresh()
    assert not L.compact and not L.compact_available
    assert np.array_equal(L.factors(), coracle.line_setup(ip, ix, d1x, p1.shape[1], 16).f)
    A.update_values(d1)
    L.refresh()
    assert L.compact and np.array_equal(L.factors(), f) and np.array_equal(L @ r, z)
    for o in (LF, K, L, F, A):
        o.close()


# ---- 3. solves ----------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("S2", "bj"), ("C1", "bj"), ("S4", "bj"), ("C0", "bj"), ("S2", "line")])
def test_solve_after_update_and_refresh(vk_lib, gpu, name, kind):
    p1 = cfg(name, 1)
    mk = (lambda A: vk_lib.block_jacobi(A, 8)) if kind == "bj" else (lambda A: vk_lib.line_jacobi(A, p1.shape[1], 16))
    A = fresh(vk_lib, gpu, name, 0)
    M = mk(A)
    A.update_vlasov(vparams(vk_lib, p1))
    M.refresh()
    b = twin.rhs(p1.n)
    x, info, st = solve(vk_lib, A, M, b)
    F = fresh(vk_lib, gpu, name, 1)
    MF = mk(F)
    xf, inf, stf = solve(vk_lib, F, MF, b)
    assert np.array_equal(x, xf), "update + refresh solves differently from a fresh operator and M"
    assert info == inf == 0 and st.inner_iters == stf.inner_iters and st.band == stf.band
    if kind == "bj" and p1.dim == 2:
        assert st.band == 1
    if p1.dim == 4:
        assert A.grid4 == tuple(p1.shape[1:])
    within_bars(x, info, st, ref_solve(name, 1, 1, kind))
    for o in (MF, M, F, A):
        o.close()


# ---- 4. a stale preconditioner ------------------------------------------------------------

@pytest.mark.parametrize("name", ["S2", "S4", "S4F", "C0"])
def test_stale_preconditioner_is_legal(vk_lib, gpu, name):
    p1 = cfg(name, 1)
    A = fresh(vk_lib, gpu, name, 0)
    M = vk_lib.block_jacobi(A, 8)
    A.update_vlasov(vparams(vk_lib, p1))
    assert (A.values_epoch, M.values_epoch) == (1, 0)
    assert np.array_equal(M.inverse(), coracle.bj_setup(*gen(name, 0), 8))   # M's own, old factors
    # (maxiter: a solve that mixed A's new values into M's old factors would not converge -- it
    # must fail here, not run 10 n cycles)
    x, info = vk_lib.gmres(A, twin.rhs(p1.n), rtol=1e-8, M=M, maxiter=100)
    st = vk_lib.last_stats()
    within_bars(x, info, st, ref_solve(name, 1, 0))
    # the lagged factors are applied as M's inverse rows; the refresh brings the requested mode back
    r = twin.rhs(p1.n, seed=5)
    assert M.mode == "inverse" and M.tridiag_available
    assert np.array_equal(M @ r, coracle.bj_apply(coracle.bj_setup(*gen(name, 0), 8), r))
    M.refresh()
    assert M.mode == "tridiag" and M.values_epoch == 1
    M.close()
    A.close()


# ---- 5. tables lost and regained ----------------------------------------------------------

def test_line_values_lost_and_regained(vk_lib, gpu):
    p1 = cfg("S2", 1)
    ip, ix, d1 = gen("S2", 1)
    assert ix[ip[167]] == 135   # row 167's first entry: its x-1 coupling
    d1x = d1.copy()
    d1x[ip[167]] *= 1.0625
    b = twin.rhs(p1.n)
    x = twin.rhs(p1.n, seed=0xC0FFEE)
    A = fresh(vk_lib, gpu, "S2", 0)
    M = vk_lib.block_jacobi(A, 8)
    assert A.line_values == 2
    A.update_values(d1x)
    M.refresh()
    assert A.line_values == 0 and A.line_band == 32
    assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1x, x))
    U = vk_lib.csr_matrix((d1x, ix, ip), shape=(p1.n, p1.n), ctx=gpu)
    MU = vk_lib.block_jacobi(U, 8)
    assert (U.line_band, U.line_values) == (32, 0)
    xa, ia, sa = solve(vk_lib, A, M, b)
    xu, iu, su = solve(vk_lib, U, MU, b)
    assert ia == iu == 0 and sa.band == su.band and np.array_equal(xa, xu)
    ref = coracle.gmres(ip, ix, d1x, b, coracle.bj_setup(ip, ix, d1x, 8), rtol=1e-8)
    within_bars(xa, ia, sa, ref)
    A.update_values(d1)
    M.refresh()
    assert A.line_values == 2 and A.values_epoch == 2
    F = fresh(vk_lib, gpu, "S2", 1)
    MF = vk_lib.block_jacobi(F, 8)
    xa, ia, sa = solve(vk_lib, A, M, b)
    xf, i_f, sf = solve(vk_lib, F, MF, b)
    assert ia == i_f == 0 and sa.band == sf.band == 1 and np.array_equal(xa, xf)
    # an uploaded CSR whose values failed at creation gains the tables with values that pass
    U.update_values(d1)
    MU.refresh()
    assert U.line_values == 2
    xu, iu, su = solve(vk_lib, U, MU, b)
    assert iu == 0 and np.array_equal(xu, xf)
    for o in (MF, MU, M, F, U, A):
        o.close()


def test_grid4_lost_and_regained(vk_lib, gpu):
    p1 = cfg("S4", 1)
    ip, ix, d1 = gen("S4", 1)
    S4 = p1.shape[1] * p1.shape[2] * p1.shape[3]
    r = 2 * S4 + 7
    assert ix[ip[r]] == r - S4   # the row's x-1 coupling
    d1x = d1.copy()
    d1x[ip[r]] *= 1.0625
    b = twin.rhs(p1.n)
    x = twin.rhs(p1.n, seed=0xC0FFEE)
    A = fresh(vk_lib, gpu, "S4", 0)
    M = vk_lib.block_jacobi(A, 8)
    assert A.grid4 == tuple(p1.shape[1:])
    A.update_values(d1x)
    M.refresh()
    assert A.grid4 == (0, 0, 0)
    assert np.array_equal(A @ x, coracle.spmv(ip, ix, d1x, x))
    U = vk_lib.csr_matrix((d1x, ix, ip), shape=(p1.n, p1.n), ctx=gpu)
    MU = vk_lib.block_jacobi(U, 8)
    assert U.grid4 == (0, 0, 0)
    xa, ia, sa = solve(vk_lib, A, M, b)
    xu, iu, su = solve(vk_lib, U, MU, b)
    assert ia == iu == 0 and np.array_equal(xa, xu)
    within_bars(xa, ia, sa, coracle.gmres(ip, ix, d1x, b, coracle.bj_setup(ip, ix, d1x, 8), rtol=1e-8))
    A.update_values(d1)
    M.refresh()
    assert A.grid4 == tuple(p1.shape[1:])
    F = fresh(vk_lib, gpu, "S4", 1)
    MF = vk_lib.block_jacobi(F, 8)
    xa, ia, sa = solve(vk_lib, A, M, b)
    xf, i_f, sf = solve(vk_lib, F, MF, b)
    assert ia == i_f == 0 and np.array_equal(xa, xf)
    U.update_values(d1)
    assert U.grid4 == tuple(p1.shape[1:])
    for o in (MF, MU, M, F, U, A):
        o.close()


# ---- 6. singular refresh ------------------------------------------------------------------

def test_singular_refresh_invalidates_until_refreshed(vk_lib, gpu):
    p1 = cfg("S2", 1)
    ip, ix, d1 = gen("S2", 1)
    dz = d1.copy()
    dz[ip[40]:ip[48]] = 0.0   # every entry of the rows of 8-block 5
    A = fresh(vk_lib, gpu, "S2", 0)
    M = vk_lib.block_jacobi(A, 8)
    L = vk_lib.line_jacobi(A, p1.shape[1], 16)
    A.update_values(dz)
    with pytest.raises(np.linalg.LinAlgError, match="singular diagonal block 5"):
        M.refresh()
    with pytest.raises(np.linalg.LinAlgError, match="zero or non-finite line pivot at row 40"):
        L.refresh()
    assert M.values_epoch == 0 and L.values_epoch == 0
    r = twin.rhs(p1.n, seed=5)
    for use in (lambda: M @ r, lambda: M.inverse(), lambda: vk_lib.gmres(A, r, M=M), lambda: A.precond_matvec(M, r),
                lambda: L @ r, lambda: L.factors(), lambda: vk_lib.gmres(A, r, M=L)):
        with pytest.raises(vk_lib._abi.VtkError) as e:
            use()
        assert e.value.status == vk_lib._abi.ERR_STATE
    with pytest.raises(np.linalg.LinAlgError):   # still singular: still invalid
        M.refresh()
    A.update_values(d1)
    M.refresh()
    L.refresh()
    assert M.values_epoch == L.values_epoch == A.values_epoch == 2
    F = fresh(vk_lib, gpu, "S2", 1)
    MF = vk_lib.block_jacobi(F, 8)
    LF = vk_lib.line_jacobi(F, p1.shape[1], 16)
    assert np.array_equal(M.inverse(), MF.inverse()) and np.array_equal(M @ r, MF @ r) and M.mode == MF.mode
    assert np.array_equal(L.factors(), LF.factors()) and np.array_equal(L @ r, LF @ r)
    for o in (LF, MF, L, M, F, A):
        o.close()


# ---- 7. across ranks ----------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _update_worker(rank, world, port, case, outdir):
    """One rank (host-staged communicator, the ranks share cuda:0): update_vlasov(p1) and refresh
    on a p0 operator, then a fresh p1 operator and preconditioner in the same worker."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    p0, p1 = cfg(case, 0), cfg(case, 1)
    align = p0.shape[1] if p0.dim == 2 else p0.shape[1] * p0.shape[2] * p0.shape[3]   # whole lines / x planes
    if p0.dim == 4:   # the LDS-ring step across ranks, as test_gpu_multirank.py runs it
        ctx.set_tuning("g4_ring", 64)
    offs = vk.partition_rows(p0.n, world, align)
    rb, re_ = int(offs[rank]), int(offs[rank + 1])
    A = vk.vlasov_operator(vparams(vk, p0), ctx=ctx, offsets=offs)
    M = vk.block_jacobi(A, 8)
    ops = len(hc.log)
    A.update_vlasov(vparams(vk, p1))
    M.refresh()
    grew = len(hc.log) - ops   # update and refresh are rank-local: no collective
    b = twin.rhs(p0.n)[rb:re_]
    xr = twin.rhs(p0.n, seed=0xC0FFEE)[rb:re_]
    y = A @ xr
    x, info = vk.gmres(A, b, rtol=1e-8, M=M)
    st = vk.last_stats()
    tabs = (A.line_band, A.line_values) + A.grid4
    gd = A.download()[2]
    F = vk.vlasov_operator(vparams(vk, p1), ctx=ctx, offsets=offs)
    MF = vk.block_jacobi(F, 8)
    yf = F @ xr
    xf, inff = vk.gmres(F, b, rtol=1e-8, M=MF)
    stf = vk.last_stats()
    np.savez(os.path.join(outdir, f"upd{rank}.npz"), rb=rb, re=re_, grew=grew, y=y, yf=yf, x=x, xf=xf, info=info,
             inff=inff, iters=st.inner_iters, itersf=stf.inner_iters, band=st.band, bandf=stf.band, gd=gd,
             tabs=np.array(tabs), tabsf=np.array((F.line_band, F.line_values) + F.grid4),
             inv=M.inverse(), invf=MF.inverse(), epochs=np.array([A.values_epoch, M.values_epoch]),
             errors=np.array(hc.errors, dtype=object).astype(str), commlog=json.dumps(hc.log))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["S2", "S4"])
def test_update_and_refresh_across_ranks(tmp_path, case):
    import torch.multiprocessing as mp

    from vtkrylov.comm import check_sequences
    world = 2
    mp.spawn(_update_worker, args=(world, _free_port(), case, str(tmp_path)), nprocs=world, join=True)
    p1 = cfg(case, 1)
    ip, ix, d1 = gen(case, 1)
    ref = ref_solve(case, 1, 1)
    inv_ref = coracle.bj_setup(ip, ix, d1, 8)
    y_ref = coracle.spmv(ip, ix, d1, twin.rhs(p1.n, seed=0xC0FFEE))
    z = [np.load(tmp_path / f"upd{r}.npz", allow_pickle=False) for r in range(world)]
    xs = np.zeros(p1.n)
    for q in z:
        rb, re_ = int(q["rb"]), int(q["re"])
        assert q["errors"].size == 0, q["errors"]
        assert int(q["grew"]) == 0, "update / refresh issued a collective"
        assert list(q["epochs"]) == [1, 1]
        assert np.array_equal(q["gd"], d1[ip[rb]:ip[re_]])
        assert np.array_equal(q["y"], q["yf"]) and np.array_equal(q["y"], y_ref[rb:re_])
        assert np.array_equal(q["inv"], q["invf"]) and np.array_equal(q["inv"], inv_ref[rb // 8:(re_ + 7) // 8])
        assert np.array_equal(q["tabs"], q["tabsf"])
        if p1.dim == 2:
            assert list(q["tabs"][:2]) == [p1.shape[1], 2] and int(q["band"]) == 1
        else:
            assert tuple(q["tabs"][2:]) == tuple(p1.shape[1:])
        assert np.array_equal(q["x"], q["xf"]), "update + refresh differs from fresh on this rank"
        assert int(q["info"]) == int(q["inff"]) == ref.info == 0
        assert int(q["iters"]) == int(q["itersf"]) and int(q["band"]) == int(q["bandf"])
        assert abs(int(q["iters"]) - ref.inner_iters) <= 1
        xs[rb:re_] = q["x"]
    assert np.linalg.norm(xs - ref.x) / np.linalg.norm(ref.x) <= 1e-9
    check_sequences([json.loads(str(q["commlog"])) for q in z])
