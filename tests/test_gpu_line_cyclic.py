"""GPU checks of the periodic whole-line preconditioner (vtkrylov.line_cyclic):
M = A's diagonal + the couplings between line neighbours modulo `period`, one cyclic tridiagonal
system per line, solved by a recursive Schur complement on separators.

References, all formed here:
* apply: a cyclic elimination in np.longdouble per line system (cyclic_solve_ld).  With err_ref
  the error of splu(M).solve -- the SciPy statement -- against it, the device's error must be
  <= 16 x max(err_ref, 2^-52 max|z|): the project's margin on the reference's own
  error, floored at one unit roundoff of the result;
* solves: twin.scipy_gmres / SciPy's bicgstab with LinearOperator(matvec=splu(M).solve) -- same
  info, iterations +-1, ||x - x_ref|| / ||x_ref|| <= 1e-9;
* one Arnoldi cycle: oracle/arnoldi.py's figures with a test-local operator at the 16x margin.
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
from test_line_cyclic_host import cyclic_matrix

pytestmark = pytest.mark.gpu

LD = np.longdouble
CASES = {
    "S2": twin.CONFIGS["S2"], "S4": twin.CONFIGS["S4"], "S4F": twin.CONFIGS["S4F"],
    "16x8": twin.Vlasov(2, (16, 8)), "50x8": twin.Vlasov(2, (50, 8)), "96x16": twin.Vlasov(2, (96, 16)),
    "16x70": twin.Vlasov(2, (16, 70)),
}


def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


def direction(p, which="x"):
    """(stride, period) of the operator's x-lines (or the 4D y-lines)."""
    if p.dim == 2:
        return p.shape[1], p.shape[0]
    if which == "y":
        return p.shape[2] * p.shape[3], p.shape[1]
    return p.shape[1] * p.shape[2] * p.shape[3], p.shape[0]


def cyclic_solve_ld(a, b, c, r, dtype=LD):
    """x with a[i] x[i-1] + b[i] x[i] + c[i] x[i+1] = r[i], indices modulo P = len(b), in
    longdouble (or dtype), every column one system: the first P - 1 unknowns eliminated (Thomas, right-hand
    sides r and the couplings to the last unknown), then the last unknown's own equation."""
    a, b, c, r = (np.asarray(v).astype(dtype) for v in (a, b, c, r))
    P = b.shape[0]
    u, y, v = b[:P - 1].copy(), r[:P - 1].copy(), np.zeros_like(r[:P - 1])
    v[0] += a[0]
    v[P - 2] += c[P - 2]
    for i in range(1, P - 1):
        f = a[i] / u[i - 1]
        u[i], y[i], v[i] = u[i] - f * c[i - 1], y[i] - f * y[i - 1], v[i] - f * v[i - 1]
    y[P - 2], v[P - 2] = y[P - 2] / u[P - 2], v[P - 2] / u[P - 2]
    for i in range(P - 3, -1, -1):
        y[i], v[i] = (y[i] - c[i] * y[i + 1]) / u[i], (v[i] - c[i] * v[i + 1]) / u[i]
    xl = (r[P - 1] - a[P - 1] * y[P - 2] - c[P - 1] * y[0]) / (b[P - 1] - a[P - 1] * v[P - 2] - c[P - 1] * v[0])
    return np.concatenate([y - v * xl, xl[None]])


class Reference:
    """M of (ip, ix, d) for (stride, period): SciPy's splu(M).solve and the longdouble solve."""

    def __init__(self, ip, ix, d, n, stride, period, dtype=LD):
        from scipy.sparse.linalg import splu
        self.n, self.S, self.P, self.dtype = n, stride, period, dtype
        self.M = cyclic_matrix(ip, ix, d, n, stride, period)
        self.lu = splu(self.M.tocsc(), permc_spec="NATURAL")
        R = np.arange(n, dtype=np.int64)
        i, blk, j = (R // stride) % period, R // (stride * period), R % stride
        nb = lambda di: (blk * period + (i + di) % period) * stride + j
        Mr = self.M.tocsr()
        self.abc = [self.lines(np.asarray(Mr[R, col]).ravel()).astype(dtype) for col in (nb(-1), R, nb(1))]

    def lines(self, v):   # (n,) -> (period, lines)
        return np.asarray(v).reshape(-1, self.P, self.S).transpose(1, 0, 2).reshape(self.P, -1)

    def unlines(self, x):
        return x.reshape(self.P, -1, self.S).transpose(1, 0, 2).reshape(-1)

    def solve_ld(self, r):
        return self.unlines(cyclic_solve_ld(*self.abc, self.lines(r), self.dtype))

    def operator(self):
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator((self.n, self.n), dtype=np.float64,
                              matvec=lambda r: self.lu.solve(np.asarray(r, np.float64).reshape(-1)))


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(p, (ip, ix, d), SciPy CSR, b) of a named operator; read-only."""
    p = CASES[name]
    csr = coracle.generate(p)
    for a in csr:
        a.setflags(write=False)
    b = twin.rhs(p.n)
    b.setflags(write=False)
    return p, csr, twin.scipy_csr(csr[0], csr[1], csr[2].astype(np.float64), p.n), b


@functools.lru_cache(maxsize=None)
def reference(name, which="x"):
    p, (ip, ix, d), _, _ = host_case(name)
    return Reference(ip, ix, d, p.n, *direction(p, which))


@functools.lru_cache(maxsize=None)
def gmres_ref(name, which="x"):
    _, _, Asp, b = host_case(name)
    ref = twin.scipy_gmres(Asp, b, reference(name, which).operator(), rtol=1e-8, restart=20)
    ref.x.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def ops(gpu, vk_lib):
    out = {name: vk_lib.vlasov_operator(vparams(vk_lib, p), ctx=gpu) for name, p in CASES.items()}
    yield out
    for A in out.values():
        A.close()


def check_apply(tag, z, r, ref):
    """The bar of the module docstring; prints both errors."""
    zl = ref.solve_ld(r)
    err_ref = float(np.abs(ref.lu.solve(np.asarray(r, np.float64)).astype(LD) - zl).max())
    err = float(np.abs(np.asarray(z).astype(LD) - zl).max())
    floor = 2.0 ** -52 * float(np.abs(zl).max())
    print(f"{tag}: device error {err:.3e}, splu error {err_ref:.3e}, 2^-52 max|z| {floor:.3e}")
    assert np.all(np.isfinite(z))
    assert err <= 16 * max(err_ref, floor), (err, err_ref, floor)


def check_solve(xg, info, iters, ref, csr, b):
    print(f"info {info} (ref {ref.info}) inner {iters} (ref {ref.inner_iters})")
    assert info == ref.info == 0
    assert abs(iters - ref.inner_iters) <= 1, (iters, ref.inner_iters)
    rel = np.linalg.norm(xg - ref.x) / np.linalg.norm(ref.x)
    print(f"x_rel {rel:.3e}")
    assert rel <= 1e-9, rel
    res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(xg)))
    assert res <= 1e-8 * np.linalg.norm(b), res / np.linalg.norm(b)


# ---- 1. apply against splu(M).solve ----------------------------------------------------------

# name, direction, seg, linec_serial (None: default), levels expected (unknowns per line)
APPLY = [
    ("S2", "x", 25, None, [64, 3]),           # ragged: 25 + 25 + 14
    ("S2", "x", 4, None, [64, 16]),
    ("S2", "x", 4, 4, [64, 16, 4]),           # three levels
    ("16x8", "x", 2, None, [16, 8]),
    ("50x8", "x", 7, None, [50, 8]),          # period no multiple of seg: 7 x 7 + 1
    ("S4", "y", 2, None, [5, 3]),             # 2 + 2 + 1
    ("S4F", "y", 2, None, [5, 3]),
    ("S4", "x", 3, None, [6, 2]),
    ("16x70", "x", 4, None, [16, 4]),         # stride 70: a full and a ragged wave of lanes
    ("S2", "x", 2, 2, [64, 32, 16, 8, 4, 2]),  # every level halves
    ("S2", "x", 12, None, [64, 6]),           # the register variants for seg <= 16 ...
    ("S2", "x", 30, None, [64, 3]),           # ... and <= 32
    ("S2", "x", 40, None, [64, 2]),           # the generic sweeps (seg > 32)
    ("S2", "x", 100, None, [64, 1]),          # one segment per line
]


@pytest.mark.parametrize("name,which,seg,serial,levels", APPLY,
                         ids=[f"{a[0]}-{a[1]}-seg{a[2]}-ser{a[3]}" for a in APPLY])
def test_apply_vs_splu(ops, gpu, vk_lib, name, which, seg, serial, levels):
    import torch
    p, _, _, b = host_case(name)
    stride, period = direction(p, which)
    if which == "x":
        prm = vparams(vk_lib, p)
        assert (vk_lib.vlasov_line_stride(prm), vk_lib.vlasov_line_period(prm)) == (stride, period)
    with gpu.tuning(**({} if serial is None else {"linec_serial": serial})):
        M = vk_lib.line_cyclic(ops[name], stride, period, seg)
    try:
        info = M.info()
        assert info["unknowns"] == levels and info["levels"] == len(levels), info
        assert (info["stride"], info["period"], info["seg"], info["compact"]) == (stride, period, seg, False)
        assert M.shape == (p.n, p.n) and M.dtype == np.float64 and M.values_epoch == ops[name].values_epoch
        ref = reference(name, which)
        for tag, r in (("rhs", b), ("rhs2", twin.rhs(p.n, seed=0xC0FFEE))):
            z = M @ r
            check_apply(f"{name} {which} seg {seg} {tag}", z, r, ref)
            assert np.array_equal(z, M @ r), "the apply is deterministic"
        zt = M.matvec(torch.from_numpy(np.array(b)).to("cuda:0"))
        assert np.array_equal(zt.cpu().numpy(), M @ b)
    finally:
        M.close()


def test_apply_dropin_csr(gpu, vk_lib):
    """The drop-in route: vk.csr_matrix of S2's arrays instead of the device assembly."""
    p, (ip, ix, d), _, b = host_case("S2")
    A = vk_lib.csr_matrix((d, ix, ip), shape=(p.n, p.n), ctx=gpu)
    M = vk_lib.line_cyclic(A, *direction(p), 25)
    try:
        check_apply("S2 drop-in", M @ b, b, reference("S2"))
    finally:
        M.close()
        A.close()


# ---- 2. the preconditioned matvec -------------------------------------------------------------

@pytest.mark.parametrize("layout", ["csr", "sell"])
@pytest.mark.parametrize("name,which,seg", [("S2", "x", 25), ("S4", "y", 2), ("S4F", "x", 3)])
def test_precond_matvec(ops, vk_lib, name, which, seg, layout):
    p = host_case(name)[0]
    A = ops[name]
    x = twin.rhs(p.n, seed=0xC0FFEE)
    which_ref = reference(name, which)
    A.set_layout(layout)
    try:
        M = vk_lib.line_cyclic(A, *direction(p, which), seg)
        y = A @ x
        w = A.precond_matvec(M, x)
        check_apply(f"{name} {layout} precond_matvec", w, y, which_ref)
        assert np.array_equal(w, M @ y)
        M.close()
    finally:
        A.set_layout("auto")


# ---- 3. solves against SciPy -------------------------------------------------------------------

SOLVES = [("S2", "x", 25), ("96x16", "x", 25), ("S4", "y", 2)]


@pytest.mark.parametrize("orth", ["mgs", "dcgs2"])
@pytest.mark.parametrize("name,which,seg", SOLVES, ids=[f"{a[0]}-{a[1]}" for a in SOLVES])
def test_gmres_vs_scipy(ops, gpu, vk_lib, name, which, seg, orth):
    p, csr, _, b = host_case(name)
    M = vk_lib.line_cyclic(ops[name], *direction(p, which), seg)
    try:
        gpu.profile(True)
        xg, info = vk_lib.gmres(ops[name], b, rtol=1e-8, M=M, orth=orth)
        st = vk_lib.last_stats()
        prof = gpu.profile_read()
        gpu.profile(False)
        check_solve(xg, info, st.inner_iters, gmres_ref(name, which), csr, b)
        if orth == "dcgs2":   # the step's form: the three phases, then the dots kernel
            for cls in ("linec_sweep", "linec_reduced", "linec_correct"):
                assert prof.get(cls, {}).get("launches", 0) > 0, sorted(prof)
    finally:
        gpu.profile(False)
        M.close()


@pytest.mark.parametrize("name", ["S2", "96x16"])
def test_half_the_iterations_of_line_jacobi(ops, vk_lib, name):
    """The wrap is what the segments of line_jacobi lose: SciPy needs 4 iterations with the cyclic
    lines against 12 with line_jacobi(A, Nv, 25) on both operators."""
    p, _, Asp, b = host_case(name)
    stride, period = direction(p)
    A = ops[name]
    M = vk_lib.line_cyclic(A, stride, period, 25)
    L = vk_lib.line_jacobi(A, stride, 25)
    try:
        _, i1 = vk_lib.gmres(A, b, rtol=1e-8, M=M)
        itc = vk_lib.last_stats().inner_iters
        _, i2 = vk_lib.gmres(A, b, rtol=1e-8, M=L)
        itj = vk_lib.last_stats().inner_iters
    finally:
        M.close()
        L.close()
    ip, ix, d = host_case(name)[1]
    refj = twin.scipy_gmres(Asp, b, twin.line_operator(ip, ix, d.astype(np.float64), p.n, stride, 25), rtol=1e-8, restart=20)
    refc = gmres_ref(name)
    print(f"{name}: line_cyclic {itc} (SciPy {refc.inner_iters}), line_jacobi {itj} (SciPy {refj.inner_iters})")
    assert i1 == i2 == 0
    assert 2 * refc.inner_iters <= refj.inner_iters
    assert 2 * itc <= itj, (itc, itj)


@pytest.mark.parametrize("name,which,seg", [("S2", "x", 25), ("S4", "y", 2)])
def test_bicgstab_vs_scipy(ops, vk_lib, name, which, seg):
    """tests/test_gpu_bicgstab.py's bars against SciPy's bicgstab with the same LinearOperator."""
    from scipy.sparse.linalg import bicgstab
    p, csr, Asp, b = host_case(name)
    rtol = 1e-8
    count = [0]
    xr, infor = bicgstab(Asp, b, rtol=rtol, atol=0.0, maxiter=500, M=reference(name, which).operator(),
                         callback=lambda _: count.__setitem__(0, count[0] + 1))
    M = vk_lib.line_cyclic(ops[name], *direction(p, which), seg)
    try:
        x, info = vk_lib.bicgstab(ops[name], b, rtol=rtol, M=M, maxiter=500)
        st = vk_lib.last_bicgstab_stats()
    finally:
        M.close()
    itr = count[0]
    print(f"info {info} (ref {infor}) iterations {st.iterations} half {st.half_step} (SciPy callbacks {itr})")
    assert info == infor == 0
    res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(x)))
    assert res <= 1.01 * rtol * np.linalg.norm(b), res
    assert abs(st.iterations - st.half_step - itr) <= max(2, math.ceil(0.15 * itr)), (st.iterations, st.half_step, itr)
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 4 * rtol


# ---- 4. the Arnoldi pin -----------------------------------------------------------------------

class CyclicOperator(ar.Operator):
    """B = M^-1 A with M the cyclic lines, solved per line in the chosen precision."""

    def __init__(self, indptr, indices, data, n, stride, period, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        self.ref = Reference(indptr, indices, data, n, stride, period, dtype)

    def Minv(self, r):
        return self.ref.solve_ld(np.asarray(r).astype(self.dtype))


ARN_M = 12


@pytest.mark.parametrize("orth", ["dcgs2", "mgs"])
def test_arnoldi_cycle_pinned(ops, gpu, vk_lib, orth):
    """One full cycle of 12 columns on S4 with the cyclic y-lines (seg 2): F1-F6 within 16x of the
    plain float64 Arnoldi on the same operator."""
    from types import SimpleNamespace
    p, _, _, b = host_case("S4")
    stride, period = direction(p, "y")
    A = ops["S4"]
    M = vk_lib.line_cyclic(A, stride, period, 2)
    ip, ix, d = A.download()
    cops = SimpleNamespace(ld=CyclicOperator(ip, ix, d, p.n, stride, period),
                           f64=CyclicOperator(ip, ix, d, p.n, stride, period, np.float64))
    dc = orth == "dcgs2"
    try:
        cyc, cap, st = _run(vk_lib, gpu, A, M, b, ARN_M, rtol=NOSTOP, maxiter=1, orth=orth)
        assert st.orth == (1 if dc else 0) and st.band == 0
        _check_full_cycle(cap, ARN_M, dc=dc)
        _compare(f"line cyclic S4-y {orth} m={ARN_M}", cops, b, cyc, "cgs2" if dc else "mgs")
    finally:
        M.close()


# ---- 5. refresh -------------------------------------------------------------------------------

def test_refresh_after_update(gpu, vk_lib):
    p0 = twin.CONFIGS["S2"]
    p1 = dataclasses.replace(p0, cfl=8.0, E0=0.8)
    stride, period = direction(p0)
    A = vk_lib.vlasov_operator(vparams(vk_lib, p0), ctx=gpu)
    M = vk_lib.line_cyclic(A, stride, period, 4)
    r = twin.rhs(p0.n)
    z0 = M @ r
    A.update_vlasov(vparams(vk_lib, p1))
    assert M.values_epoch == 0 and A.values_epoch == 1
    assert np.array_equal(M @ r, z0), "without refresh() the old factors apply (a lagged M)"
    assert M.refresh() is M and M.values_epoch == 1
    F = vk_lib.line_cyclic(A, stride, period, 4)
    z1 = M @ r
    assert np.array_equal(z1, F @ r) and not np.array_equal(z1, z0)
    ip, ix, d = coracle.generate(p1)
    check_apply("S2 refreshed", z1, r, Reference(ip, ix, d, p1.n, stride, period))
    for o in (F, M, A):
        o.close()


def test_refresh_singular_then_good(gpu, vk_lib):
    """A zero diagonal planted by update_values: refresh() raises LinAlgError naming the row and M
    is unusable (ERR_STATE) until a refresh from good values."""
    import scipy.sparse as sp
    n, stride, period = 24, 3, 8
    Asp = sp.diags([-0.75, -1.0, -0.5, 4.0, -0.25, -0.75, -1.0], [-21, -3, -1, 0, 1, 3, 21], shape=(n, n), format="csr")
    ip, ix, d = Asp.indptr.astype(np.int32), Asp.indices.astype(np.int32), Asp.data.copy()
    A = vk_lib.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu)
    M = vk_lib.line_cyclic(A, stride, period, 4)
    r = twin.rhs(n)
    ref = Reference(ip, ix, d, n, stride, period)
    check_apply("banded 24", M @ r, r, ref)
    bad = d.copy()
    bad[ip[0] + np.flatnonzero(ix[ip[0]:ip[1]] == 0)[0]] = 0.0
    A.update_values(bad)
    with pytest.raises(np.linalg.LinAlgError, match="row 0 "):
        M.refresh()
    for call in (lambda: M @ r, lambda: vk_lib.gmres(A, r, M=M), lambda: A.precond_matvec(M, r)):
        with pytest.raises(vk_lib._abi.VtkError) as e:
            call()
        assert e.value.status == vk_lib._abi.ERR_STATE
    A.update_values(d)
    M.refresh()
    check_apply("banded 24 after a good refresh", M @ r, r, ref)
    M.close()
    A.close()


# ---- 6. ranks sharing one GPU (host-staged communicator) --------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    out = {}
    # S4 in slabs of three x-planes: every cyclic y-line lies on one rank
    p = twin.CONFIGS["S4"]
    sx = p.shape[1] * p.shape[2] * p.shape[3]
    offs = vk.partition_rows(p.n, world, sx)
    rb, re_ = int(offs[rank]), int(offs[rank + 1])
    A = vk.vlasov_operator(vparams(vk, p), ctx=ctx, offsets=offs)
    M = vk.line_cyclic(A, *direction(p, "y"), 2)
    b = twin.rhs(p.n)
    out["z"] = M @ b[rb:re_]
    for orth in ("dcgs2", "mgs"):
        x, info = vk.gmres(A, b[rb:re_], rtol=1e-8, M=M, orth=orth)
        out.update({f"x_{orth}": x, f"info_{orth}": info, f"it_{orth}": vk.last_stats().inner_iters})
    # the 2D x-lines span the ranks: refused
    p2 = twin.CONFIGS["S2"]
    offs2 = vk.partition_rows(p2.n, world, p2.shape[1])
    A2 = vk.vlasov_operator(vparams(vk, p2), ctx=ctx, offsets=offs2)
    try:
        vk.line_cyclic(A2, *direction(p2), 25)
        out["refused"] = 0
    except ValueError:
        out["refused"] = 1
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), **out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_sharing_one_gpu(ops, vk_lib, tmp_path):
    import torch.multiprocessing as mp
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    p, csr, _, b = host_case("S4")
    ref = reference("S4", "y")
    M = vk_lib.line_cyclic(ops["S4"], *direction(p, "y"), 2)
    z1 = M @ b
    M.close()
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    zz, xs = np.zeros(p.n), {k: np.zeros(p.n) for k in ("dcgs2", "mgs")}
    for r in range(world):
        assert z[r]["errors"].size == 0, z[r]["errors"]
        assert int(z[r]["refused"]) == 1, "S2's x-lines across two ranks must be VTK_ERR_ARG"
        rb, re_ = int(z[r]["rb"]), int(z[r]["re"])
        assert (rb, re_) == (r * p.n // 2, (r + 1) * p.n // 2)
        zz[rb:re_] = z[r]["z"]
        for k in xs:
            xs[k][rb:re_] = z[r][f"x_{k}"]
            assert int(z[r][f"info_{k}"]) == int(z[0][f"info_{k}"]) and int(z[r][f"it_{k}"]) == int(z[0][f"it_{k}"])
    check_apply("S4-y two ranks", zz, b, ref)
    check_apply("S4-y one rank", z1, b, ref)
    for k in xs:
        check_solve(xs[k], int(z[0][f"info_{k}"]), int(z[0][f"it_{k}"]), gmres_ref("S4", "y"), csr, b)


# ---- 7. errors --------------------------------------------------------------------------------

def test_errors(ops, gpu, vk_lib):
    import ctypes as C
    vk = vk_lib
    p = host_case("S2")[0]
    A = ops["S2"]
    stride, period = direction(p)
    for args in ((stride, 2, 25), (stride, period, 1), (stride, period, 0), (0, period, 25), (stride, -1, 25),
                 (stride, period - 1, 25),       # n is no multiple of stride * period
                 (stride + 1, period, 25)):
        with pytest.raises(ValueError):
            vk.line_cyclic(A, *args)
    M = vk.line_cyclic(A, stride, period, 25)
    L = vk.line_jacobi(A, stride, 25)
    lib, h = vk._abi.lib(), A.ctx.handle
    u = C.c_int()
    f = np.empty(3 * p.n)
    fp = f.ctypes.data_as(C.c_void_p)
    for call in (lambda: lib.vtk_linejacobi_get_compact(M.handle, C.byref(u), None),
                 lambda: lib.vtk_linejacobi_set_compact(M.handle, 0),
                 lambda: lib.vtk_linejacobi_factors(M.handle, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_lineproduct_factors(M.handle, 0, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_bjacobi_inverse(M.handle, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_linecyclic_info(L.handle, C.byref(vk._abi.LinecInfo()))):
        with pytest.raises(vk._abi.VtkError) as e:
            vk._abi.check(call(), h)
        assert e.value.status == vk._abi.ERR_STATE
    k = C.c_int()
    vk._abi.check(lib.vtk_prec_kind_of(M.handle, C.byref(k)), h)
    assert k.value == 3
    with pytest.raises((ValueError, vk._abi.VtkError)):
        vk.gmres(ops["96x16"], twin.rhs(CASES["96x16"].n), M=M)
    with pytest.raises(TypeError, match="LineCyclic"):
        vk.gmres(A, twin.rhs(p.n), M=object())
    M.close()
    L.close()
