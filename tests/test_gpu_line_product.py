"""GPU parity of the two-direction line preconditioner (vtkrylov.line_product):
M = M1 D^-1 M2 with M1, M2 two line-Jacobi matrices of A and D A's diagonal, applied as
z = M2^-1 (D .* (M1^-1 r)).

References, all formed here from what oracle/ already has:
* factors of direction i: coracle.line_setup(ip, ix, d, stride_i, seg_i).f, bit for bit;
* D: the stored-order sum of each row's diagonal entries, bit for bit;
* apply: coracle.line_apply(lf2, D * coracle.line_apply(lf1, r)), bit for bit, and
  splu(M2).solve(D * splu(M1).solve(r)) (twin.line_matrix) within the line bar rtol 1e-12 /
  atol 1e-14;
* GMRES: twin.scipy_gmres with that LinearOperator -- same info, inner iterations +-1,
  ||x - x_ref|| / ||x_ref|| <= 1e-9, true residual <= 1e-8 ||b||;
* BiCGStab: SciPy's bicgstab with the same LinearOperator, tests/test_gpu_bicgstab.py's bars;
* one Arnoldi cycle: oracle/arnoldi.py's figures with a test-local product operator, the
  project's 16x margin (tests/test_gpu_arnoldi_steps.py's comparison).
"""
import dataclasses
import functools
import math
import os
import socket

import numpy as np
import pytest

from oracle import arnoldi as ar
from oracle import coracle, twin
from test_gpu_arnoldi_steps import NOSTOP, _check_full_cycle, _compare, _run

pytestmark = pytest.mark.gpu

P4 = twin.Vlasov(4, (50, 25, 6, 5), fp32=True)      # the issue's third GMRES operator
SEGS = [(1, 1), (3, 5), (8, 16), (25, 25), (32, 40), (40, 1 << 30)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def strides_of(p):
    if p.dim == 2:
        return p.shape[1], 1
    return p.shape[1] * p.shape[2] * p.shape[3], p.shape[2] * p.shape[3]


def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


def diag_sum(ip, ix, d, row0=0):
    """Per row the sum of its stored entries with col == row, in stored order from 0.0."""
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(ip, np.int64))) + row0
    m = np.asarray(ix, np.int64) == rows
    D = np.zeros(n)
    np.add.at(D, rows[m] - row0, np.asarray(d)[m].astype(np.float64))
    return D


def chained(lf1, lf2, D, r):
    return coracle.line_apply(lf2, D * coracle.line_apply(lf1, np.ascontiguousarray(r)))


def scipy_product(ip, ix, d, n, d1, d2):
    """The SciPy statement: LinearOperator(matvec=lambda r: lu2.solve(D * lu1.solve(r)))."""
    from scipy.sparse.linalg import LinearOperator, splu
    lu1 = splu(twin.line_matrix(ip, ix, d, n, *d1).tocsc(), permc_spec="NATURAL")
    lu2 = splu(twin.line_matrix(ip, ix, d, n, *d2).tocsc(), permc_spec="NATURAL")
    D = diag_sum(ip, ix, d)
    return LinearOperator((n, n), matvec=lambda r: lu2.solve(D * lu1.solve(np.asarray(r, np.float64).reshape(-1))),
                          dtype=np.float64)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(p, (ip, ix, d), SciPy CSR, b) of a named operator; read-only."""
    p = P4 if name == "P4" else twin.CONFIGS[name]
    csr = coracle.generate(p)
    for a in csr:
        a.setflags(write=False)
    b = twin.rhs(p.n)
    b.setflags(write=False)
    return p, csr, twin.scipy_csr(csr[0], csr[1], csr[2].astype(np.float64), p.n), b


@functools.lru_cache(maxsize=None)
def gmres_ref(name, segs):
    p, (ip, ix, d), Asp, b = host_case(name)
    s1, s2 = strides_of(p)
    ref = twin.scipy_gmres(Asp, b, scipy_product(ip, ix, d, p.n, (s1, segs[0]), (s2, segs[1])), rtol=1e-8, restart=20)
    ref.x.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def ops(gpu, vk_lib):
    out = {}
    for name in ("S4", "S4F", "S2", "P4"):
        p = host_case(name)[0]
        out[name] = vk_lib.vlasov_operator(vparams(vk_lib, p), ctx=gpu)
    yield out
    for A in out.values():
        A.close()


def check_solve(xg, info, iters, ref, csr, b):
    print(f"info {info} (ref {ref.info}) inner {iters} (ref {ref.inner_iters})")
    assert info == ref.info == 0
    assert abs(iters - ref.inner_iters) <= 1, (iters, ref.inner_iters)
    rel = np.linalg.norm(xg - ref.x) / np.linalg.norm(ref.x)
    print(f"x_rel {rel:.3e}")
    assert rel <= 1e-9, rel
    res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(xg)))
    assert res <= 1e-8 * np.linalg.norm(b), res / np.linalg.norm(b)


# ---- 1. factors and apply, bit-exact; 2. apply against SciPy ---------------------------------

def _bitexact(vk, A, csr, n, d1, d2, scipy_too):
    import torch
    ip, ix, d = csr
    r = twin.rhs(n)
    D = diag_sum(ip, ix, d)
    lf = [coracle.line_setup(ip, ix, d, *dd) for dd in (d1, d2)]
    for (a, b_), (la, lb) in (((d1, d2), (lf[0], lf[1])), ((d2, d1), (lf[1], lf[0]))):   # and swapped
        M = vk.line_product(A, a, b_)
        try:
            assert M.shape == (n, n) and M.dtype == np.float64 and M.values_epoch == A.values_epoch
            assert np.array_equal(bits(M.factors(0)), bits(la.f))
            assert np.array_equal(bits(M.factors(1)), bits(lb.f))
            assert np.array_equal(bits(M.diagonal()), bits(D))
            z = M @ r
            assert np.array_equal(bits(z), bits(chained(la, lb, D, r)))
            zt = M.matvec(torch.from_numpy(r).to("cuda:0"))
            assert np.array_equal(bits(zt.cpu().numpy()), bits(z))
            if scipy_too and (a, b_) == (d1, d2):
                np.testing.assert_allclose(z, scipy_product(ip, ix, d, n, d1, d2).matvec(r), rtol=1e-12, atol=1e-14)
        finally:
            M.close()


BITEXACT = [(name, segs) for name in ("S4", "S4F", "S2") for segs in SEGS] + [("S4", (3, 2))]


@pytest.mark.parametrize("name,segs", BITEXACT, ids=[f"{n}-{s[0]}-{s[1]}" for n, s in BITEXACT])
def test_factors_and_apply_bitexact(ops, vk_lib, name, segs):
    """Every register variant (seg <= 8 / 16 / 25 / 32) and the generic sweep (> 32) in both
    positions (the swapped product runs the other kernel on each direction).  (3, 2) on S4: 2 does
    not divide Ny = 5, the y segments straddle x-planes, where the coupling is absent."""
    p, csr, _, _ = host_case(name)
    s1, s2 = strides_of(p)
    assert vk_lib.vlasov_line_directions(vparams(vk_lib, p)) == [s1, s2]
    _bitexact(vk_lib, ops[name], csr, p.n, (s1, segs[0]), (s2, segs[1]), scipy_too=True)


@pytest.mark.parametrize("segs", SEGS, ids=lambda s: f"{s[0]}-{s[1]}")
def test_ragged_csr_bitexact(gpu, vk_lib, golden, segs):
    """A general CSR (no constant couplings: the stored-factor sweeps), strides (37, 5)."""
    ip, ix, d = golden["ragged/indptr"], golden["ragged/indices"], golden["ragged/data"]
    n = ip.shape[0] - 1
    A = vk_lib.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu)
    try:
        _bitexact(vk_lib, A, (ip, ix, d), n, (37, segs[0]), (5, segs[1]), scipy_too=True)
    finally:
        A.close()


# ---- 3. the fused step ------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["csr", "sell"])
@pytest.mark.parametrize("name", ["S4", "S4F", "S2"])
def test_precond_matvec_bitexact(ops, vk_lib, name, layout):
    p = host_case(name)[0]
    A = ops[name]
    s1, s2 = strides_of(p)
    x = twin.rhs(p.n, seed=0xC0FFEE)
    A.set_layout(layout)
    try:
        M = vk_lib.line_product(A, (s1, 3), (s2, 5))
        assert np.array_equal(bits(A.precond_matvec(M, x)), bits(M @ (A @ x)))
        M.close()
    finally:
        A.set_layout("auto")


@pytest.mark.parametrize("name,segs", [("S4", (3, 5)), ("S4F", (25, 25)), ("S2", (8, 16))])
def test_line2_dc_settings(ops, gpu, vk_lib, name, segs):
    """DCGS2 with the dots behind the second sweep (line2_dc 1) and with the plain second sweep
    followed by the dots kernel (0): both within the solve bars, each deterministic, and the
    profile shows which kernels ran."""
    p, csr, _, b = host_case(name)
    s1, s2 = strides_of(p)
    M = vk_lib.line_product(ops[name], (s1, segs[0]), (s2, segs[1]))
    ref = gmres_ref(name, segs)
    try:
        for dc, cls, other in ((1, "line2_dc", "line2_sweep"), (0, "line2_sweep", "line2_dc")):
            with gpu.tuning(line2_dc=dc):
                assert gpu.get_tuning("line2_dc") == dc
                gpu.profile(True)
                x1, i1 = vk_lib.gmres(ops[name], b, rtol=1e-8, M=M, orth="dcgs2")
                it1 = vk_lib.last_stats().inner_iters
                prof = gpu.profile_read()
                gpu.profile(False)
                x2, i2 = vk_lib.gmres(ops[name], b, rtol=1e-8, M=M, orth="dcgs2")
            assert prof.get(cls, {}).get("launches", 0) > 0 and other not in prof, sorted(prof)
            assert prof.get("line_apply", {}).get("launches", 0) > 0, sorted(prof)
            check_solve(x1, i1, it1, ref, csr, b)
            assert i2 == i1 and np.array_equal(bits(x1), bits(x2))
    finally:
        M.close()


# ---- 4. GMRES against SciPy; 5. stronger than one direction ----------------------------------

GM = [("S4", (3, 5)), ("S4", (25, 25)), ("S4F", (3, 5)), ("S4F", (25, 25)), ("P4", (25, 25))]


@pytest.mark.parametrize("orth", ["mgs", "dcgs2"])
@pytest.mark.parametrize("name,segs", GM, ids=[f"{n}-{s[0]}-{s[1]}" for n, s in GM])
def test_gmres_vs_scipy(ops, vk_lib, name, segs, orth):
    p, csr, _, b = host_case(name)
    s1, s2 = strides_of(p)
    M = vk_lib.line_product(ops[name], (s1, segs[0]), (s2, segs[1]))
    try:
        xg, info = vk_lib.gmres(ops[name], b, rtol=1e-8, M=M, orth=orth)
        check_solve(xg, info, vk_lib.last_stats().inner_iters, gmres_ref(name, segs), csr, b)
    finally:
        M.close()


@pytest.mark.parametrize("name,segs", [("S4", (3, 5)), ("P4", (25, 25))])
def test_product_stronger_than_one_direction(ops, vk_lib, name, segs):
    """Device iterations with the product <= 0.6 x device iterations with line Jacobi on direction
    1 (CPU: 28 / 54 = 0.52 on S4, 19 / 37 = 0.51 on (50,25,6,5); +-1 on both stays <= 0.56)."""
    p, _, _, b = host_case(name)
    s1, s2 = strides_of(p)
    A = ops[name]
    M = vk_lib.line_product(A, (s1, segs[0]), (s2, segs[1]))
    L = vk_lib.line_jacobi(A, s1, segs[0])
    try:
        _, i2 = vk_lib.gmres(A, b, rtol=1e-8, M=M)
        it2 = vk_lib.last_stats().inner_iters
        _, i1 = vk_lib.gmres(A, b, rtol=1e-8, M=L)
        it1 = vk_lib.last_stats().inner_iters
    finally:
        M.close()
        L.close()
    print(f"{name}: product {it2}, line-x {it1}, ratio {it2 / it1:.3f}")
    assert i1 == i2 == 0
    assert it2 <= 0.6 * it1, (it2, it1)


# ---- 6. BiCGStab ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S4", "S4F"])
def test_bicgstab_vs_scipy(ops, vk_lib, name):
    """tests/test_gpu_bicgstab.py's bars against SciPy's bicgstab with the same LinearOperator
    (SciPy's callback count is iterations - half_step)."""
    from scipy.sparse.linalg import bicgstab
    p, csr, Asp, b = host_case(name)
    ip, ix, d = csr
    s1, s2 = strides_of(p)
    rtol = 1e-8
    count = [0]
    xr, infor = bicgstab(Asp, b, rtol=rtol, atol=0.0, maxiter=500, M=scipy_product(ip, ix, d, p.n, (s1, 3), (s2, 5)),
                         callback=lambda _: count.__setitem__(0, count[0] + 1))
    M = vk_lib.line_product(ops[name], (s1, 3), (s2, 5))
    try:
        x, info = vk_lib.bicgstab(ops[name], b, rtol=rtol, M=M, maxiter=500)
        st = vk_lib.last_bicgstab_stats()
    finally:
        M.close()
    itr = count[0]
    print(f"info {info} (ref {infor}) iterations {st.iterations} half {st.half_step} (SciPy callbacks {itr})")
    assert info == infor == 0
    atol_eff = rtol * np.linalg.norm(b)
    res = np.linalg.norm(b - coracle.spmv(ip, ix, d, np.ascontiguousarray(x)))
    assert res <= 1.01 * atol_eff, (res, atol_eff)
    assert abs(st.iterations - st.half_step - itr) <= max(2, math.ceil(0.15 * itr)), (st.iterations, st.half_step, itr)
    rel = np.linalg.norm(x - xr) / np.linalg.norm(xr)
    assert rel <= 4 * rtol, rel


# ---- 7. refresh -------------------------------------------------------------------------------

def test_refresh_after_update(gpu, vk_lib):
    p0 = twin.CONFIGS["S4"]
    p1 = dataclasses.replace(p0, cfl=8.0, E0=0.8)
    s1, s2 = strides_of(p0)
    A = vk_lib.vlasov_operator(vparams(vk_lib, p0), ctx=gpu)
    M = vk_lib.line_product(A, (s1, 3), (s2, 5))
    r = twin.rhs(p0.n)
    z0 = M @ r
    A.update_vlasov(vparams(vk_lib, p1))
    assert M.values_epoch == 0 and A.values_epoch == 1
    assert np.array_equal(bits(M @ r), bits(z0)), "without refresh() the old factors apply (a lagged M)"
    assert M.refresh() is M and M.values_epoch == 1
    F = vk_lib.line_product(A, (s1, 3), (s2, 5))
    for w in (0, 1):
        assert np.array_equal(bits(M.factors(w)), bits(F.factors(w)))
    assert np.array_equal(bits(M.diagonal()), bits(F.diagonal()))
    z1 = M @ r
    assert np.array_equal(bits(z1), bits(F @ r)) and not np.array_equal(z1, z0)
    ip, ix, d = coracle.generate(p1)
    D = diag_sum(ip, ix, d)
    assert np.array_equal(bits(z1), bits(chained(coracle.line_setup(ip, ix, d, s1, 3),
                                                 coracle.line_setup(ip, ix, d, s2, 5), D, r)))
    for o in (F, M, A):
        o.close()


def test_refresh_singular_then_good(gpu, vk_lib):
    """A zero diagonal planted by update_values: refresh() raises LinAlgError and M is unusable
    (ERR_STATE) until a refresh from good values."""
    import scipy.sparse as sp
    n = 24
    Asp = sp.diags([-1.0, -0.5, 4.0, -0.25, -0.75], [-6, -1, 0, 1, 6], shape=(n, n), format="csr")
    ip, ix, d = Asp.indptr.astype(np.int32), Asp.indices.astype(np.int32), Asp.data.copy()
    A = vk_lib.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu)
    M = vk_lib.line_product(A, (6, 2), (1, 3))
    r = twin.rhs(n)
    bad = d.copy()
    bad[np.flatnonzero(ix[:ip[1]] == 0)[0]] = 0.0         # row 0's diagonal: a first pivot in both directions
    A.update_values(bad)
    with pytest.raises(np.linalg.LinAlgError):
        M.refresh()
    for call in (lambda: M @ r, lambda: M.factors(0), lambda: M.diagonal(), lambda: vk_lib.gmres(A, r, M=M)):
        with pytest.raises(vk_lib._abi.VtkError) as e:
            call()
        assert e.value.status == vk_lib._abi.ERR_STATE
    A.update_values(d)
    M.refresh()
    D = diag_sum(ip, ix, d)
    assert np.array_equal(bits(M @ r), bits(chained(coracle.line_setup(ip, ix, d, 6, 2),
                                                    coracle.line_setup(ip, ix, d, 1, 3), D, r)))
    M.close()
    A.close()


# ---- 8. ranks sharing one GPU (host-staged communicator) --------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, seg1, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    p = twin.CONFIGS["S4"]
    s1, s2 = strides_of(p)
    offs = vk.partition_rows(p.n, world, s1)
    rb, re_ = int(offs[rank]), int(offs[rank + 1])
    A = vk.vlasov_operator(vparams(vk, p), ctx=ctx, offsets=offs)
    M = vk.line_product(A, (s1, seg1), (s2, 5))
    b = twin.rhs(p.n)
    out = dict(f0=M.factors(0), f1=M.factors(1), D=M.diagonal(), z=M @ b[rb:re_])
    for orth in ("dcgs2", "mgs"):
        x, info = vk.gmres(A, b[rb:re_], rtol=1e-8, M=M, orth=orth)
        out.update({f"x_{orth}": x, f"info_{orth}": info, f"it_{orth}": vk.last_stats().inner_iters})
    x, info = vk.bicgstab(A, b[rb:re_], rtol=1e-8, M=M, maxiter=500)
    st = vk.last_bicgstab_stats()
    out.update(x_bcg=x, info_bcg=info, it_bcg=st.iterations, half_bcg=st.half_step)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,seg1", [(2, 3), (3, 2)])
def test_ranks_sharing_one_gpu(tmp_path, world, seg1):
    """S4 (Nx = 6) in x-plane slabs: seg1 = 3 at world 2 and 2 at world 3 divide every rank's
    x-range, and y lines never cross a slab, so M is the one-rank M."""
    import torch.multiprocessing as mp
    from scipy.sparse.linalg import bicgstab
    mp.spawn(_worker, args=(world, _free_port(), seg1, str(tmp_path)), nprocs=world, join=True)
    p, csr, Asp, b = host_case("S4")
    ip, ix, d = csr
    s1, s2 = strides_of(p)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    xs = {k: np.zeros(p.n) for k in ("dcgs2", "mgs", "bcg")}
    for r in range(world):
        assert z[r]["errors"].size == 0, z[r]["errors"]
        rb, re_ = int(z[r]["rb"]), int(z[r]["re"])
        bip, bix, bd = coracle.generate(p, rb, re_)
        lf1 = coracle.line_setup(bip, bix, bd, s1, seg1, row0=rb)
        lf2 = coracle.line_setup(bip, bix, bd, s2, 5, row0=rb)
        D = diag_sum(bip, bix, bd, row0=rb)
        assert np.array_equal(bits(z[r]["f0"]), bits(lf1.f)) and np.array_equal(bits(z[r]["f1"]), bits(lf2.f))
        assert np.array_equal(bits(z[r]["D"]), bits(D))
        assert np.array_equal(bits(z[r]["z"]), bits(chained(lf1, lf2, D, b[rb:re_])))
        for k in xs:
            xs[k][rb:re_] = z[r][f"x_{k}"]
            assert int(z[r][f"info_{k}"]) == int(z[0][f"info_{k}"]) and int(z[r][f"it_{k}"]) == int(z[0][f"it_{k}"])
        assert int(z[r]["half_bcg"]) == int(z[0]["half_bcg"])
    ref = twin.scipy_gmres(Asp, b, scipy_product(ip, ix, d, p.n, (s1, seg1), (s2, 5)), rtol=1e-8, restart=20)
    for k in ("dcgs2", "mgs"):
        check_solve(xs[k], int(z[0][f"info_{k}"]), int(z[0][f"it_{k}"]), ref, csr, b)
    count = [0]
    xr, infor = bicgstab(Asp, b, rtol=1e-8, atol=0.0, maxiter=500, M=scipy_product(ip, ix, d, p.n, (s1, seg1), (s2, 5)),
                         callback=lambda _: count.__setitem__(0, count[0] + 1))
    itb = int(z[0]["it_bcg"]) - int(z[0]["half_bcg"])
    assert int(z[0]["info_bcg"]) == infor == 0
    assert np.linalg.norm(b - coracle.spmv(ip, ix, d, xs["bcg"])) <= 1.01e-8 * np.linalg.norm(b)
    assert abs(itb - count[0]) <= max(2, math.ceil(0.15 * count[0])), (itb, count[0])
    assert np.linalg.norm(xs["bcg"] - xr) / np.linalg.norm(xr) <= 4e-8


# ---- 9. the Arnoldi pin -----------------------------------------------------------------------

class ProductOperator(ar.Operator):
    """B = M^-1 A with M^-1 r = M2^-1 (D (M1^-1 r)): two line operators of oracle.arnoldi around
    the diagonal multiply, in the chosen precision."""

    def __init__(self, indptr, indices, data, n, d1, d2, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        self.l1 = ar.Operator(indptr, indices, data, n, ("line",) + tuple(d1), dtype)
        self.l2 = ar.Operator(indptr, indices, data, n, ("line",) + tuple(d2), dtype)
        self.D = diag_sum(indptr, indices, data).astype(dtype)

    def Minv(self, r):
        return self.l2.Minv(self.D * self.l1.Minv(r))


ARN_M = 12


@pytest.mark.parametrize("mode", ["dcgs2-dc1", "dcgs2-dc0", "mgs"])
def test_arnoldi_cycle_pinned(ops, gpu, vk_lib, mode):
    """One full cycle of 12 columns on S4 with the product (3, 5): F1-F6 within 16x of the plain
    float64 Arnoldi on the same operator."""
    from types import SimpleNamespace
    p, _, _, b = host_case("S4")
    s1, s2 = strides_of(p)
    A = ops["S4"]
    M = vk_lib.line_product(A, (s1, 3), (s2, 5))
    ip, ix, d = A.download()
    pops = SimpleNamespace(ld=ProductOperator(ip, ix, d, p.n, (s1, 3), (s2, 5)),
                           f64=ProductOperator(ip, ix, d, p.n, (s1, 3), (s2, 5), np.float64))
    dc = mode != "mgs"
    try:
        with gpu.tuning(line2_dc=0 if mode.endswith("dc0") else 1):
            cyc, cap, st = _run(vk_lib, gpu, A, M, b, ARN_M, rtol=NOSTOP, maxiter=1, orth="dcgs2" if dc else "mgs")
        assert st.orth == (1 if dc else 0) and st.band == 0
        _check_full_cycle(cap, ARN_M, dc=dc)
        _compare(f"line product S4 {mode} m={ARN_M}", pops, b, cyc, "cgs2" if dc else "mgs")
    finally:
        M.close()


# ---- 10. errors -------------------------------------------------------------------------------

def test_errors(ops, gpu, vk_lib):
    vk = vk_lib
    p = host_case("S4")[0]
    A = ops["S4"]
    s1, s2 = strides_of(p)
    for d1, d2 in (((0, 3), (s2, 5)), ((s1, 0), (s2, 5)), ((s1, 3), (0, 5)), ((s1, 3), (s2, 0)),
                   ((p.n, 3), (s2, 5)), ((s1, 3), (p.n, 5))):
        with pytest.raises(ValueError):
            vk.line_product(A, d1, d2)
    M = vk.line_product(A, (s1, 3), (s2, 5))
    L = vk.line_jacobi(A, s1, 3)
    lib, h = vk._abi.lib(), A.ctx.handle
    import ctypes as C
    u = C.c_int()
    with pytest.raises(vk._abi.VtkError) as e:
        vk._abi.check(lib.vtk_linejacobi_get_compact(M.handle, C.byref(u), None), h)
    assert e.value.status == vk._abi.ERR_STATE
    f = np.empty(3 * p.n)
    with pytest.raises(vk._abi.VtkError) as e:
        vk._abi.check(lib.vtk_lineproduct_factors(L.handle, 0, f.ctypes.data_as(C.c_void_p), vk._abi.PTR_HOST), h)
    assert e.value.status == vk._abi.ERR_STATE
    with pytest.raises(ValueError):
        M.factors(2)
    k = C.c_int()
    vk._abi.check(lib.vtk_prec_kind_of(M.handle, C.byref(k)), h)
    assert k.value == 2
    other = ops["S4F"]
    with pytest.raises((ValueError, vk._abi.VtkError)):
        vk.gmres(other, twin.rhs(p.n), M=M)
    with pytest.raises(TypeError, match="LineProduct"):
        vk.gmres(A, twin.rhs(p.n), M=object())
    with pytest.raises(TypeError, match="LineProduct"):
        vk.bicgstab(A, twin.rhs(p.n), M=object())
    with pytest.raises(TypeError, match="LineProduct"):
        A.precond_matvec(object(), twin.rhs(p.n))
    M.close()
    L.close()
