"""GPU checks of the Neumann-series wrapper (vtkrylov.neumann)

    N_k^-1 r :  z_1 = M^-1 r ;  z_{i+1} = z_i + M^-1 (r - A z_i),  i = 1 .. k-1

around every base preconditioner M.  References, all formed here:
* apply, bases block Jacobi / line Jacobi / line product: the unfused composition of the library's own
  ``A @ x`` and ``M @ x`` with NumPy's double subtraction and addition, bit for bit (the contract of
  include/vtkrylov.h), whichever kernels the wrapper runs;
* apply, base line_cyclic: the SciPy statement evaluated in np.longdouble here; the device error
  must be <= 16 x max(the float64 SciPy statement's own error against it, 2^-52 max|z|);
* solves: twin.scipy_gmres / SciPy's bicgstab with the SciPy statement as LinearOperator -- same
  info, inner iterations +-1, ||x - x_ref|| / ||x_ref|| <= 1e-9;
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
from test_gpu_line_cyclic import Reference as CyclicReference
from test_gpu_line_product import diag_sum, scipy_product
from test_neumann_host import neumann_mv, neumann_operator

pytestmark = pytest.mark.gpu

LD = np.longdouble
DEGREES = (1, 2, 3, 4, 8)
CASES = {"S2": twin.CONFIGS["S2"], "16x8": twin.Vlasov(2, (16, 8)), "S4": twin.CONFIGS["S4"], "S4F": twin.CONFIGS["S4F"]}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


def strides_of(p):
    if p.dim == 2:
        return p.shape[1], 1
    return p.shape[1] * p.shape[2] * p.shape[3], p.shape[2] * p.shape[3]


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


@pytest.fixture(scope="module")
def ops(gpu, vk_lib, golden):
    out = {name: vk_lib.vlasov_operator(vparams(vk_lib, p), ctx=gpu) for name, p in CASES.items()}
    ip, ix, d = golden["ragged/indptr"], golden["ragged/indices"], golden["ragged/data"]
    out["ragged"] = vk_lib.csr_matrix((d, ix, ip), shape=(ip.shape[0] - 1,) * 2, ctx=gpu)
    yield out
    for A in out.values():
        A.close()


# the bases: name -> (constructor from (vk, A, strides), the operators it runs on)
def _line_strides(name):
    return (37, 5) if name == "ragged" else strides_of(CASES[name])


def make_base(vk, A, name, base):
    s1, s2 = _line_strides(name)
    kind, *arg = base.split("-")
    if kind == "bj":
        return vk.block_jacobi(A, int(arg[0]), mode=arg[1] if len(arg) > 1 else "auto")
    if kind == "line":
        return vk.line_jacobi(A, s1, int(arg[0]))
    if kind == "product":
        return vk.line_product(A, (s1, 3), (s2, 5))
    raise KeyError(base)


def composition(A, M, r, degrees):
    """degree -> the unfused composition: the device's A @ x and M @ x, NumPy's double - and +."""
    out, z = {}, M @ r
    for k in range(1, max(degrees) + 1):
        if k > 1:
            z = z + (M @ (r - (A @ z)))
        if k in degrees:
            out[k] = z
    return out


# ---- 1. apply, bit for bit --------------------------------------------------------------------

BJ_BASES = ["bj-1-inverse", "bj-4-inverse", "bj-4-tridiag", "bj-8-inverse", "bj-8-tridiag", "bj-16"]
LINE_BASES = ["line-25", "line-8", "line-40", "product"]
APPLY = [(name, base) for name in ("S2", "16x8", "S4", "S4F", "ragged") for base in BJ_BASES + LINE_BASES
         if not (name == "ragged" and base.endswith("tridiag"))]     # ragged blocks are not tridiagonal


@pytest.mark.parametrize("name,base", APPLY, ids=[f"{a}-{b}" for a, b in APPLY])
def test_apply_bitexact(ops, gpu, vk_lib, name, base):
    """Degrees 1-4 and 8 in both layouts, and for block Jacobi with the one-launch correction (neu_fuse
    1, where the tiles allow it) and the three-launch form (0): all equal to the composition."""
    import torch
    A = ops[name]
    n = A.n_local
    r = twin.rhs(n, seed=0xC0FFEE)
    try:
        for layout in ("csr", "sell"):
            A.set_layout(layout)
            M = make_base(vk_lib, A, name, base)
            try:
                ref = composition(A, M, r, DEGREES)
                for fuse in ((1, 0) if base.startswith("bj") else (1,)):
                    with gpu.tuning(neu_fuse=fuse):
                        for k in DEGREES:
                            N = vk_lib.neumann(A, M, k)
                            info = N.info()
                            assert info["degree"] == k and info["base_alive"] and N.values_epoch == M.values_epoch
                            assert N.shape == (n, n) and N.dtype == np.float64
                            if base.startswith("bj") and k > 1:
                                bs = int(base.split("-")[1])
                                # one launch per correction: bs <= 8 on BJ-fused tiles, and not switched off
                                # (a general CSR's stream tiles may not align with the blocks: either form)
                                if not (name == "ragged" and layout == "csr" and fuse and bs <= 8):
                                    assert info["fused"] == bool(fuse and bs <= 8), (info, layout)
                            else:
                                assert not info["fused"]
                            z = N @ r
                            assert np.array_equal(bits(z), bits(ref[k])), (layout, fuse, k, np.abs(z - ref[k]).max())
                            if k in (1, 3):
                                zt = N.matvec(torch.from_numpy(r).to("cuda:0"))
                                assert np.array_equal(bits(zt.cpu().numpy()), bits(z))
                            N.close()
                # degree 1 is the base
                assert np.array_equal(bits(ref[1]), bits(M @ r))
            finally:
                M.close()
    finally:
        A.set_layout("auto")


# ---- 2. the line_cyclic base: to rounding -------------------------------------------------------

def _A_ld(csr, x):
    ip, ix, d = csr
    return np.add.reduceat(np.asarray(d).astype(LD) * np.asarray(x).astype(LD)[np.asarray(ix, np.int64)],
                           np.asarray(ip, np.int64)[:-1])


@pytest.mark.parametrize("seg", [25, 4])
def test_apply_line_cyclic(ops, vk_lib, seg):
    """S2's periodic x-lines as the base.  The reference is the recursion in longdouble (the line
    systems by test_gpu_line_cyclic's cyclic elimination, A's rows summed in longdouble)."""
    p, csr, Asp, b = host_case("S2")
    stride, period = p.shape[1], p.shape[0]
    cref = CyclicReference(*csr, p.n, stride, period)
    M = vk_lib.line_cyclic(ops["S2"], stride, period, seg)
    try:
        for tag, r in (("rhs", b), ("rhs2", twin.rhs(p.n, seed=0xC0FFEE))):
            zl = cref.solve_ld(r)
            for k in range(1, max(DEGREES) + 1):
                if k > 1:
                    zl = zl + cref.solve_ld(np.asarray(r).astype(LD) - _A_ld(csr, zl))
                if k not in DEGREES:
                    continue
                zs = neumann_mv(Asp, cref.lu.solve, k)(r)
                N = vk_lib.neumann(ops["S2"], M, k)
                z = N @ r
                N.close()
                err_ref = float(np.abs(zs.astype(LD) - zl).max())
                err = float(np.abs(np.asarray(z).astype(LD) - zl).max())
                floor = 2.0 ** -52 * float(np.abs(zl).max())
                print(f"S2 line_cyclic seg {seg} {tag} degree {k}: device error {err:.3e}, SciPy statement error {err_ref:.3e}, "
                      f"2^-52 max|z| {floor:.3e}")
                assert np.all(np.isfinite(z))
                assert err <= 16 * max(err_ref, floor), (k, err, err_ref, floor)
                if k == 1:
                    assert np.array_equal(bits(z), bits(M @ r)), "degree 1 is the base, bit for bit"
    finally:
        M.close()


# ---- 3. the preconditioned matvec ---------------------------------------------------------------

@pytest.mark.parametrize("layout", ["csr", "sell"])
@pytest.mark.parametrize("name,base", [("S2", "bj-8-tridiag"), ("S4F", "bj-8-inverse"), ("S4", "product"), ("S2", "line-25"),
                                       ("ragged", "bj-16")])
def test_precond_matvec_bitexact(ops, vk_lib, name, base, layout):
    A = ops[name]
    x = twin.rhs(A.n_local, seed=0xC0FFEE)
    A.set_layout(layout)
    try:
        M = make_base(vk_lib, A, name, base)
        for k in (1, 2, 3):
            N = vk_lib.neumann(A, M, k)
            assert np.array_equal(bits(A.precond_matvec(N, x)), bits(N @ (A @ x))), k
            N.close()
        M.close()
    finally:
        A.set_layout("auto")


# ---- 4. solves against SciPy ------------------------------------------------------------------------

def scipy_base(name, base):
    """M^-1 of the SciPy statement for a base of the solve tests, as a callable."""
    p, (ip, ix, d), _, _ = host_case(name)
    d64 = np.asarray(d, np.float64)
    s1, s2 = strides_of(p)
    if base == "bj-8":
        Binv = twin.bj_inverse_numpy(ip, ix, d64, p.n, 8)
        return lambda r: twin.bj_apply_numpy(Binv, r, p.n)
    if base == "line-25":
        return twin.line_operator(ip, ix, d64, p.n, s1, 25).matvec
    if base == "product":
        return scipy_product(ip, ix, d, p.n, (s1, 3), (s2, 5)).matvec
    if base == "cyclic":
        return CyclicReference(ip, ix, d, p.n, p.shape[1], p.shape[0]).lu.solve
    raise KeyError(base)


def device_base(vk, A, name, base):
    p = CASES[name]
    if base == "bj-8":
        return vk.block_jacobi(A, 8)
    if base == "cyclic":
        return vk.line_cyclic(A, p.shape[1], p.shape[0], 25)
    return make_base(vk, A, name, base)


# BJ(8) at degree 3 does not converge on these operators (eigenvalues of M^-1 A outside
# the unit disc around 1); three restart cycles of it are compared like any other solve, info = 3
MAXITER = {("bj-8", 3): 3}
SOLVES = [("S2", "bj-8"), ("S2", "line-25"), ("S4", "product"), ("S2", "cyclic")]


@functools.lru_cache(maxsize=None)
def gmres_ref(name, base, k):
    p, _, Asp, b = host_case(name)
    op = neumann_operator(Asp, scipy_base(name, base), p.n, k)
    ref = twin.scipy_gmres(Asp, b, op, rtol=1e-8, restart=20, maxiter=MAXITER.get((base, k)))
    ref.x.setflags(write=False)
    return ref


def check_solve(xg, info, iters, ref, csr, b):
    print(f"info {info} (ref {ref.info}) inner {iters} (ref {ref.inner_iters})")
    assert info == ref.info
    assert abs(iters - ref.inner_iters) <= 1, (iters, ref.inner_iters)
    rel = np.linalg.norm(xg - ref.x) / np.linalg.norm(ref.x)
    print(f"x_rel {rel:.3e}")
    assert rel <= 1e-9, rel
    if ref.info == 0:
        res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(xg)))
        assert res <= 1e-8 * np.linalg.norm(b), res / np.linalg.norm(b)


@pytest.mark.parametrize("mode", ["mgs", "dcgs2-dc1", "dcgs2-dc0"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name,base", SOLVES, ids=[f"{a}-{b}" for a, b in SOLVES])
def test_gmres_vs_scipy(ops, gpu, vk_lib, name, base, k, mode):
    p, csr, _, b = host_case(name)
    A = ops[name]
    M = device_base(vk_lib, A, name, base)
    N = vk_lib.neumann(A, M, k)
    dc = mode != "mgs"
    try:
        with gpu.tuning(neu_dc=0 if mode.endswith("dc0") else 1):
            gpu.profile(True)
            xg, info = vk_lib.gmres(A, b, rtol=1e-8, M=N, orth="dcgs2" if dc else "mgs", maxiter=MAXITER.get((base, k)))
            st = vk_lib.last_stats()
            prof = gpu.profile_read()
            gpu.profile(False)
        assert st.band == 0 and st.orth == (1 if dc else 0)
        check_solve(xg, info, st.inner_iters, gmres_ref(name, base, k), csr, b)
        # which kernels ran: one launch per correction for BJ(8); residual + the base's sweeps else
        assert prof.get("neu_corr", {}).get("launches", 0) > 0, sorted(prof)
        assert ("neu_resid" in prof) == (base != "bj-8"), sorted(prof)
        if dc and base in ("line-25", "product"):
            # the step's dots behind the last correction (neu_dc 1), or the dots kernel after it (0);
            # a cycle's closing reduction is a dots launch of its own in both settings
            steps, dots = prof["spmv"]["launches"], prof.get("dc_dots", {}).get("launches", 0)
            assert (dots >= steps) if mode.endswith("dc0") else (dots < steps), (mode, steps, dots)
    finally:
        gpu.profile(False)
        N.close()
        M.close()


@pytest.mark.parametrize("name,base,k", [("S4", "product", 2), ("S2", "bj-8", 2), ("S2", "cyclic", 3)])
def test_bicgstab_vs_scipy(ops, vk_lib, name, base, k):
    """tests/test_gpu_bicgstab.py's bars against SciPy's bicgstab with the same LinearOperator."""
    from scipy.sparse.linalg import bicgstab
    p, csr, Asp, b = host_case(name)
    rtol = 1e-8
    count = [0]
    xr, infor = bicgstab(Asp, b, rtol=rtol, atol=0.0, maxiter=500, M=neumann_operator(Asp, scipy_base(name, base), p.n, k),
                         callback=lambda _: count.__setitem__(0, count[0] + 1))
    M = device_base(vk_lib, ops[name], name, base)
    N = vk_lib.neumann(ops[name], M, k)
    try:
        x, info = vk_lib.bicgstab(ops[name], b, rtol=rtol, M=N, maxiter=500)
        st = vk_lib.last_bicgstab_stats()
    finally:
        N.close()
        M.close()
    itr = count[0]
    print(f"info {info} (ref {infor}) iterations {st.iterations} half {st.half_step} (SciPy callbacks {itr})")
    assert info == infor == 0
    res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(x)))
    assert res <= 1.01 * rtol * np.linalg.norm(b), res
    assert abs(st.iterations - st.half_step - itr) <= max(2, math.ceil(0.15 * itr)), (st.iterations, st.half_step, itr)
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 4 * rtol


@pytest.mark.parametrize("name,base", [("S2", "bj-8"), ("S4", "product")])
def test_iteration_benefit_follows_scipy(ops, vk_lib, name, base):
    """No fixed ratio to the base is asserted: the device counts of the base and of degree 2 are each
    within one of SciPy's for the same operator, so the benefit is SciPy's (BJ(8) on S2: 68 -> 35, the
    product on S4: 28 -> 16 on the CPU)."""
    p, _, _, b = host_case(name)
    A = ops[name]
    M = device_base(vk_lib, A, name, base)
    N = vk_lib.neumann(A, M, 2)
    try:
        vk_lib.gmres(A, b, rtol=1e-8, M=M)
        it1 = vk_lib.last_stats().inner_iters
        vk_lib.gmres(A, b, rtol=1e-8, M=N)
        it2 = vk_lib.last_stats().inner_iters
    finally:
        N.close()
        M.close()
    r1, r2 = gmres_ref(name, base, 1).inner_iters, gmres_ref(name, base, 2).inner_iters
    print(f"{name} {base}: device {it1} -> {it2}, SciPy {r1} -> {r2}")
    assert abs(it1 - r1) <= 1 and abs(it2 - r2) <= 1
    assert r2 < r1 and it2 < it1


# ---- 5. the Arnoldi pin -----------------------------------------------------------------------------

class NeumannOperator(ar.Operator):
    """B = N_k^-1 A around oracle.arnoldi's own block Jacobi, in the chosen precision."""

    def __init__(self, indptr, indices, data, n, bs, degree, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        self.base = ar.Operator(indptr, indices, data, n, ("bj", bs), dtype)
        self.degree = degree

    def Minv(self, r):
        r = np.asarray(r).astype(self.dtype)
        z = self.base.Minv(r)
        for _ in range(self.degree - 1):
            z = z + self.base.Minv(r - self.A(z))
        return z


ARN_M = 12


@pytest.mark.parametrize("mode", ["dcgs2", "mgs"])
def test_arnoldi_cycle_pinned(ops, gpu, vk_lib, mode):
    """One full cycle of 12 columns on S2 with BJ(8) at degree 2: F1-F6 within 16x of the plain
    float64 Arnoldi on the same operator."""
    from types import SimpleNamespace
    p, _, _, b = host_case("S2")
    A = ops["S2"]
    M = vk_lib.block_jacobi(A, 8)
    N = vk_lib.neumann(A, M, 2)
    ip, ix, d = A.download()
    nops = SimpleNamespace(ld=NeumannOperator(ip, ix, d, p.n, 8, 2), f64=NeumannOperator(ip, ix, d, p.n, 8, 2, np.float64))
    dc = mode == "dcgs2"
    try:
        cyc, cap, st = _run(vk_lib, gpu, A, N, b, ARN_M, rtol=NOSTOP, maxiter=1, orth=mode)
        assert st.orth == (1 if dc else 0) and st.band == 0
        _check_full_cycle(cap, ARN_M, dc=dc)
        _compare(f"neumann BJ(8) degree 2 S2 {mode} m={ARN_M}", nops, b, cyc, "cgs2" if dc else "mgs")
    finally:
        N.close()
        M.close()


# ---- 6. ranks sharing one GPU (host-staged communicator) ------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


RANK_CASES = {"S2": ("bj-8", 2), "S4": ("product", 3)}     # operator -> (base, degree)


def _rank_base(vk, A, name, world):
    p = CASES[name]
    s1, s2 = strides_of(p)
    if name == "S2":
        return vk.block_jacobi(A, 8)
    return vk.line_product(A, (s1, 6 // world), (s2, 5))    # x segments that divide every rank's planes


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    out = {}
    for name, (base, k) in RANK_CASES.items():
        p = CASES[name]
        offs = vk.partition_rows(p.n, world, strides_of(p)[0])
        rb, re_ = int(offs[rank]), int(offs[rank + 1])
        A = vk.vlasov_operator(vparams(vk, p), ctx=ctx, offsets=offs)
        M = _rank_base(vk, A, name, world)
        N = vk.neumann(A, M, k)
        b = twin.rhs(p.n)
        out[f"{name}_rb"], out[f"{name}_re"] = rb, re_
        out[f"{name}_z"] = N @ b[rb:re_]
        for orth in ("dcgs2", "mgs"):
            x, info = vk.gmres(A, b[rb:re_], rtol=1e-8, M=N, orth=orth)
            st = vk.last_stats()
            out.update({f"{name}_x_{orth}": x, f"{name}_info_{orth}": info, f"{name}_it_{orth}": st.inner_iters,
                        f"{name}_band_{orth}": st.band})
        x, info = vk.bicgstab(A, b[rb:re_], rtol=1e-8, M=N, maxiter=500)
        out.update({f"{name}_x_bcg": x, f"{name}_info_bcg": info})
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), errors=np.array(hc.errors, dtype=object).astype(str), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_sharing_one_gpu(ops, vk_lib, tmp_path, world):
    """S2 / BJ(8) degree 2 and S4 / line product degree 3 in x-slabs on two and three ranks: the apply
    equals the one-rank apply bit for bit (every correction exchanged its halo), the solves meet the
    one-rank bars."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    for name, (base, k) in RANK_CASES.items():
        p, csr, Asp, b = host_case(name)
        ip, ix, d = csr
        s1, s2 = strides_of(p)
        M = _rank_base(vk_lib, ops[name], name, world)
        N = vk_lib.neumann(ops[name], M, k)
        z1 = N @ b
        N.close()
        M.close()
        zz, xs = np.zeros(p.n), {key: np.zeros(p.n) for key in ("dcgs2", "mgs", "bcg")}
        for r in range(world):
            assert z[r]["errors"].size == 0, z[r]["errors"]
            rb, re_ = int(z[r][f"{name}_rb"]), int(z[r][f"{name}_re"])
            zz[rb:re_] = z[r][f"{name}_z"]
            for key in xs:
                xs[key][rb:re_] = z[r][f"{name}_x_{key}"]
                assert int(z[r][f"{name}_info_{key}"]) == int(z[0][f"{name}_info_{key}"])
            for key in ("dcgs2", "mgs"):
                assert int(z[r][f"{name}_it_{key}"]) == int(z[0][f"{name}_it_{key}"]) and int(z[r][f"{name}_band_{key}"]) == 0
        assert np.array_equal(bits(zz), bits(z1)), (name, world, np.abs(zz - z1).max())
        if name == "S2":
            Minv = scipy_base("S2", "bj-8")
        else:
            Minv = scipy_product(ip, ix, d, p.n, (s1, 6 // world), (s2, 5)).matvec
        ref = twin.scipy_gmres(Asp, b, neumann_operator(Asp, Minv, p.n, k), rtol=1e-8, restart=20)
        for key in ("dcgs2", "mgs"):
            check_solve(xs[key], int(z[0][f"{name}_info_{key}"]), int(z[0][f"{name}_it_{key}"]), ref, csr, b)
        assert int(z[0][f"{name}_info_bcg"]) == 0
        assert np.linalg.norm(b - coracle.spmv(ip, ix, d, xs["bcg"])) <= 1.01e-8 * np.linalg.norm(b)


# ---- 7. refresh and lifetime ------------------------------------------------------------------------

@pytest.mark.parametrize("base", ["bj-8-tridiag", "line-25"])
def test_refresh_follows_the_base(gpu, vk_lib, base):
    p0 = twin.CONFIGS["S2"]
    p1 = dataclasses.replace(p0, cfl=8.0, E0=0.8)
    A = vk_lib.vlasov_operator(vparams(vk_lib, p0), ctx=gpu)
    M = make_base(vk_lib, A, "S2", base)
    N = vk_lib.neumann(A, M, 2)
    r = twin.rhs(p0.n)
    z0 = N @ r
    assert np.array_equal(bits(z0), bits(composition(A, M, r, (2,))[2]))
    A.update_vlasov(vparams(vk_lib, p1))
    assert N.values_epoch == M.values_epoch == 0 and A.values_epoch == 1
    # a stale wrapper: the operator's new values in the residual, the base's old factors -- applied
    # as a stale base applies them (block Jacobi: its inverse rows), in the fused launch too
    if base.startswith("bj"):
        assert M.mode == "inverse"
    zs = N @ r
    assert np.array_equal(bits(zs), bits(composition(A, M, r, (2,))[2])) and not np.array_equal(zs, z0)
    xs, infos = vk_lib.gmres(A, r, rtol=1e-8, M=N, maxiter=2)       # solving with the lagged wrapper is legal
    assert infos in (0, 2) and np.all(np.isfinite(xs)) and vk_lib.last_stats().band == 0
    assert N.refresh() is N and N.values_epoch == 1 and M.values_epoch == 1
    if base.startswith("bj"):
        assert M.mode == "tridiag"
    F = make_base(vk_lib, A, "S2", base)
    z1 = N @ r
    assert np.array_equal(bits(z1), bits(composition(A, F, r, (2,))[2])) and not np.array_equal(z1, zs)
    # a base refreshed on its own is seen by the wrapper at its next use
    A.update_vlasov(vparams(vk_lib, p0))
    M.refresh()
    assert N.values_epoch == 2 and np.array_equal(bits(N @ r), bits(z0))
    for o in (N, F, M, A):
        o.close()


def test_refresh_singular_then_good(gpu, vk_lib):
    """A zero diagonal planted by update_values: the wrapper's refresh() raises the base's LinAlgError
    (its row) and the wrapper is unusable (ERR_STATE) until a refresh from good values."""
    import scipy.sparse as sp
    n = 24
    Asp = sp.diags([-1.0, -0.5, 4.0, -0.25, -0.75], [-6, -1, 0, 1, 6], shape=(n, n), format="csr")
    ip, ix, d = Asp.indptr.astype(np.int32), Asp.indices.astype(np.int32), Asp.data.copy()
    A = vk_lib.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu)
    M = vk_lib.line_jacobi(A, 6, 2)
    N = vk_lib.neumann(A, M, 2)
    r = twin.rhs(n)
    z0 = N @ r
    bad = d.copy()
    bad[ip[1] + np.flatnonzero(ix[ip[1]:ip[2]] == 1)[0]] = 0.0      # row 1's diagonal: the first pivot of its segment
    A.update_values(bad)
    with pytest.raises(np.linalg.LinAlgError, match=r"row 1\b"):
        N.refresh()
    for call in (lambda: N @ r, lambda: M @ r, lambda: vk_lib.gmres(A, r, M=N), lambda: vk_lib.bicgstab(A, r, M=N),
                 lambda: A.precond_matvec(N, r)):
        with pytest.raises(vk_lib._abi.VtkError) as e:
            call()
        assert e.value.status == vk_lib._abi.ERR_STATE
    A.update_values(d)
    N.refresh()
    assert np.array_equal(bits(N @ r), bits(z0))
    for o in (N, M, A):
        o.close()


def test_lifetime_and_errors(ops, gpu, vk_lib):
    import ctypes as C
    vk = vk_lib
    A = ops["S2"]
    p = CASES["S2"]
    r = twin.rhs(p.n)
    lib, h = vk._abi.lib(), A.ctx.handle
    M = vk.block_jacobi(A, 8)
    for degree in (0, 9, -3):
        with pytest.raises(ValueError, match="degree"):
            vk.neumann(A, M, degree)
    N = vk.neumann(A, M, 2)
    with pytest.raises(ValueError, match="wrapper"):       # no nesting
        vk.neumann(A, N, 2)
    with pytest.raises(ValueError, match="another operator"):
        vk.neumann(ops["16x8"], M, 2)
    with pytest.raises(TypeError, match="BlockJacobi"):
        vk.neumann(A, object(), 2)
    k = C.c_int()
    vk._abi.check(lib.vtk_prec_kind_of(N.handle, C.byref(k)), h)
    assert k.value == 4
    # the kind-specific accessors refuse the wrapper
    u = C.c_int()
    f = np.empty(64 * p.n)
    fp = f.ctypes.data_as(C.c_void_p)
    for call in (lambda: lib.vtk_linejacobi_get_compact(N.handle, C.byref(u), None),
                 lambda: lib.vtk_linejacobi_set_compact(N.handle, 0),
                 lambda: lib.vtk_linejacobi_factors(N.handle, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_lineproduct_factors(N.handle, 0, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_linecyclic_info(N.handle, C.byref(vk._abi.LinecInfo())),
                 lambda: lib.vtk_bjacobi_inverse(N.handle, fp, vk._abi.PTR_HOST),
                 lambda: lib.vtk_bjacobi_set_mode(N.handle, 1),
                 lambda: lib.vtk_bjacobi_get_mode(N.handle, C.byref(u), None),
                 lambda: lib.vtk_neumann_info(M.handle, C.byref(vk._abi.NeuInfo()))):
        with pytest.raises(vk._abi.VtkError) as e:
            vk._abi.check(call(), h)
        assert e.value.status == vk._abi.ERR_STATE
    with pytest.raises((ValueError, vk._abi.VtkError)):
        vk.gmres(ops["16x8"], twin.rhs(CASES["16x8"].n), M=N)
    with pytest.raises(TypeError, match="Neumann"):
        vk.gmres(A, r, M=object())
    # the wrapper borrows its base: closing the wrapper leaves the base usable ...
    zb = M @ r
    N2 = vk.neumann(A, M, 3)
    N2.close()
    assert np.array_equal(bits(M @ r), bits(zb))
    # ... and a wrapper whose base was closed is refused at every use, a new preconditioner at the
    # same address included
    z = N @ r
    M.close()
    M2 = vk.block_jacobi(A, 8)
    assert not N.info()["base_alive"]
    for call in (lambda: N @ r, lambda: vk.gmres(A, r, M=N), lambda: vk.bicgstab(A, r, M=N), lambda: A.precond_matvec(N, r),
                 lambda: N.refresh()):
        with pytest.raises(vk._abi.VtkError) as e:
            call()
        assert e.value.status == vk._abi.ERR_STATE
    N3 = vk.neumann(A, M2, 2)
    assert np.array_equal(bits(N3 @ r), bits(z))
    for o in (N3, N, M2):
        o.close()


# ---- 8. the band path is left alone -------------------------------------------------------------------

def test_band_path_unchanged(ops, vk_lib):
    """BJ(8) on S2 takes the line-band step, the wrapper around it does not; creating and using a
    wrapper changes nothing in the base's own solve (the same bits before and after)."""
    p, csr, _, b = host_case("S2")
    A = ops["S2"]
    M = vk_lib.block_jacobi(A, 8)
    x0, i0 = vk_lib.gmres(A, b, rtol=1e-8, M=M, orth="dcgs2")
    st0 = vk_lib.last_stats()
    assert i0 == 0 and st0.band == 1
    N = vk_lib.neumann(A, M, 2)
    xn, i_n = vk_lib.gmres(A, b, rtol=1e-8, M=N, orth="dcgs2")
    assert i_n == 0 and vk_lib.last_stats().band == 0
    N1 = vk_lib.neumann(A, M, 1)                            # degree 1: the base's operator, not its band path
    x1, i1 = vk_lib.gmres(A, b, rtol=1e-8, M=N1, orth="dcgs2")
    assert i1 == 0 and vk_lib.last_stats().band == 0
    assert abs(vk_lib.last_stats().inner_iters - st0.inner_iters) <= 1
    x2, i2 = vk_lib.gmres(A, b, rtol=1e-8, M=M, orth="dcgs2")
    st2 = vk_lib.last_stats()
    assert i2 == 0 and st2.band == 1 and st2.inner_iters == st0.inner_iters
    assert np.array_equal(bits(x2), bits(x0))
    for o in (N, N1, M):
        o.close()


# ---- 9. the vtsetup element ---------------------------------------------------------------------------

def test_vtsetup_neumann_degree(gpu, tmp_path):
    """preconditioner/neumann_degree through the entry layer: one rank in this process, then run/gpus = 2
    through test_main (two rank processes on the host-staged transport) -- as for the base kind."""
    import json
    import subprocess
    import sys
    from vtsetup.config import DEFAULT_XML, SolverConfig
    from vtsetup.krylov_precondition import KrylovPrecondition
    xml = tmp_path / "c.xml"
    xml.write_text(open(DEFAULT_XML).read().replace("</line_segment>", "</line_segment><neumann_degree>2</neumann_degree>", 1))
    base = KrylovPrecondition(SolverConfig.load(config="S2", report=str(tmp_path / "r0.json")), ctx=gpu).main()
    cfg = SolverConfig.load(str(xml), config="S2", report=str(tmp_path / "r1.json"))
    step = KrylovPrecondition(cfg, ctx=gpu)
    r1 = step.main()
    x1 = np.asarray(step.x)
    assert r1["preconditioner"]["neumann_degree"] == 2 and "neumann_degree" not in base["preconditioner"]
    assert r1["solve"]["info"] == 0 and not r1["solve"]["band_step"] and base["solve"]["band_step"]
    assert abs(r1["solve"]["inner_iters"] - gmres_ref("S2", "bj-8", 2).inner_iters) <= 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "vt-precondition_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, root]))
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, "-m", "vtsetup.krylov_precondition", "--xml", str(xml), "--config", "S2", "--gpus", "2",
                          "--comm", "host", "--report", str(tmp_path / "r2.json"), "--x-out", str(tmp_path / "x2.npy")],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r2 = json.load(open(tmp_path / "r2.json"))
    x2 = np.load(tmp_path / "x2.npy")
    assert r2["ranks"] == 2 and r2["preconditioner"]["neumann_degree"] == 2 and r2["solve"]["info"] == 0
    assert abs(r2["solve"]["inner_iters"] - r1["solve"]["inner_iters"]) <= 1 and not r2["solve"]["band_step"]
    assert np.max(np.abs(x2 - x1)) <= 1e-8 * np.max(np.abs(x1))
