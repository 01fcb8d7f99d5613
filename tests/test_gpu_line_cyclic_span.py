"""GPU checks of the cyclic lines that span the ranks (vtkrylov.line_cyclic(..., span=True);
DESIGN.md §3o): the same M as the plain kind, solved as SPIKE over ranks on top of the rank's open
chunk.  References and bars are tests/test_gpu_line_cyclic.py's, imported from there: the
longdouble elimination per line at 16 x max(splu's own error, 2^-52 max|z|) for an apply
(check_apply), SciPy with LinearOperator(matvec=splu(M).solve) for the solves (check_solve; the
BiCGStab bars of tests/test_gpu_bicgstab.py).

One rank runs the very same path with world 1 (the entry does not delegate to the plain kind), so
every new kernel is exercised in this process; ranks that share the GPU go through the host-staged
communicator over gloo, one mp.spawn per world."""
import ctypes as C
import dataclasses
import datetime
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import coracle, twin
from test_gpu_line_cyclic import (CASES, Reference, _free_port, check_apply, check_solve, direction, gmres_ref,
                                  host_case, ops, reference, vparams)  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu


def bicgstab_ref(name):
    from scipy.sparse.linalg import bicgstab
    _, _, Asp, b = host_case(name)
    count = [0]
    xr, info = bicgstab(Asp, b, rtol=1e-8, atol=0.0, maxiter=500, M=reference(name).operator(),
                        callback=lambda _: count.__setitem__(0, count[0] + 1))
    return xr, info, count[0]


def check_bicgstab(name, x, info, iterations, half_step):
    """tests/test_gpu_line_cyclic.py::test_bicgstab_vs_scipy's bars."""
    _, csr, _, b = host_case(name)
    xr, infor, itr = bicgstab_ref(name)
    print(f"{name}: info {info} (ref {infor}) iterations {iterations} half {half_step} (SciPy callbacks {itr})")
    assert info == infor == 0
    res = np.linalg.norm(b - coracle.spmv(*csr, np.ascontiguousarray(x)))
    assert res <= 1.01 * 1e-8 * np.linalg.norm(b), res
    assert abs(iterations - half_step - itr) <= max(2, math.ceil(0.15 * itr)), (iterations, half_step, itr)
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 4 * 1e-8


# ---- 1. one rank: the spike path with world 1 -------------------------------------------------------

# name, seg, linec_serial (None: default), the chunk's levels (unknowns per line)
APPLY = [
    ("S2", 25, None, [64, 3]),
    ("S2", 4, 4, [64, 16, 4]),        # three levels
    ("S2", 12, None, [64, 6]),        # the register variants for seg <= 16 ...
    ("S2", 30, None, [64, 3]),        # ... and <= 32
    ("S2", 40, None, [64, 2]),        # the generic loops (seg > 32)
    ("S2", 100, None, [64, 1]),       # one segment per line: the one-level local solve
    ("16x8", 2, None, [16, 8]),
    ("50x8", 7, None, [50, 8]),       # 7 x 7 + 1
    ("S4", 3, None, [6, 2]),          # the 4D x-lines
    ("S4F", 3, None, [6, 2]),
    ("16x70", 4, None, [16, 4]),      # stride 70: a full and a ragged wave of lanes
]


@pytest.mark.parametrize("name,seg,serial,levels", APPLY, ids=[f"{a[0]}-seg{a[1]}-ser{a[2]}" for a in APPLY])
def test_apply_world1(ops, gpu, vk_lib, name, seg, serial, levels):
    p, _, _, b = host_case(name)
    stride, period = direction(p)
    with gpu.tuning(**({} if serial is None else {"linec_serial": serial})):
        M = vk_lib.line_cyclic(ops[name], stride, period, seg, span=True)
    try:
        info = M.info()
        assert info["unknowns"] == levels and info["levels"] == len(levels), info
        assert (info["stride"], info["period"], info["seg"]) == (stride, period, seg)
        assert M.span and M.span_info == {"world": 1, "rank": 0, "first_line": 0, "local_period": period,
                                          "period": period, "spanning": True}
        ref = reference(name)
        for tag, r in (("rhs", b), ("rhs2", twin.rhs(p.n, seed=0xC0FFEE))):
            z = M @ r
            check_apply(f"{name} span seg {seg} {tag}", z, r, ref)
            assert np.array_equal(z, M @ r), "the apply is deterministic"
    finally:
        M.close()


def test_plain_kind_reports_no_span(ops, vk_lib):
    p = host_case("S2")[0]
    M = vk_lib.line_cyclic(ops["S2"], *direction(p), 25)
    try:
        assert not M.span
        with pytest.raises(vk_lib._abi.VtkError) as e:
            M.span_info
        assert e.value.status == vk_lib._abi.ERR_STATE
    finally:
        M.close()


# ---- 2. one rank: the matvec, the solves, the one-rank RCCL communicator -------------------------------

@pytest.mark.parametrize("layout", ["csr", "sell"])
def test_precond_matvec(ops, vk_lib, layout):
    p = host_case("S2")[0]
    A = ops["S2"]
    x = twin.rhs(p.n, seed=0xC0FFEE)
    A.set_layout(layout)
    try:
        M = vk_lib.line_cyclic(A, *direction(p), 25, span=True)
        y = A @ x
        w = A.precond_matvec(M, x)
        check_apply(f"S2 {layout} span precond_matvec", w, y, reference("S2"))
        assert np.array_equal(w, M @ y)
        M.close()
    finally:
        A.set_layout("auto")


@pytest.mark.parametrize("orth", ["mgs", "dcgs2"])
def test_gmres_vs_scipy(ops, gpu, vk_lib, orth):
    p, csr, _, b = host_case("S2")
    M = vk_lib.line_cyclic(ops["S2"], *direction(p), 25, span=True)
    try:
        gpu.profile(True)
        xg, info = vk_lib.gmres(ops["S2"], b, rtol=1e-8, M=M, orth=orth)
        st = vk_lib.last_stats()
        prof = gpu.profile_read()
        gpu.profile(False)
        check_solve(xg, info, st.inner_iters, gmres_ref("S2"), csr, b)
        if orth == "dcgs2":   # the step's form: the chunk's two phases, the rank level, the fused correction
            for cls in ("linec_sweep", "linec_reduced", "linec_span", "linec_correct_span"):
                assert prof.get(cls, {}).get("launches", 0) > 0, sorted(prof)
            assert "linec_correct" not in prof
    finally:
        gpu.profile(False)
        M.close()


def test_bicgstab_vs_scipy(ops, vk_lib):
    p, _, _, b = host_case("S2")
    M = vk_lib.line_cyclic(ops["S2"], *direction(p), 25, span=True)
    try:
        x, info = vk_lib.bicgstab(ops["S2"], b, rtol=1e-8, M=M, maxiter=500)
        st = vk_lib.last_bicgstab_stats()
    finally:
        M.close()
    check_bicgstab("S2", x, info, st.iterations, st.half_step)


def test_rccl_solo_apply(vk_lib):
    """The same apply on a one-rank RCCL communicator (tests/test_gpu_rccl_solo.py): the setup's and
    the apply's gathers go through ncclAllGather."""
    os.environ["VTK_COMM_SOLO"] = "1"
    try:
        ctx = vk_lib.Context(0)
        ctx.comm_init(0, 1, vk_lib.Context.unique_id())
    finally:
        del os.environ["VTK_COMM_SOLO"]
    p, _, _, b = host_case("S2")
    A = vk_lib.vlasov_operator(vparams(vk_lib, p), ctx=ctx)
    M = vk_lib.line_cyclic(A, *direction(p), 25, span=True)
    try:
        assert M.span_info["world"] == 1
        z = M @ b
        check_apply("S2 span, one-rank RCCL", z, b, reference("S2"))
        xg, info = vk_lib.gmres(A, b, rtol=1e-8, M=M)
        check_solve(xg, info, vk_lib.last_stats().inner_iters, gmres_ref("S2"), host_case("S2")[1], b)
    finally:
        M.close()
        A.close()


# ---- 3.-5. ranks sharing the GPU (host-staged communicator) ---------------------------------------------

# key, operator, seg, linec_serial, drop-in CSR
RANK_CASES = {
    2: [("s2", "S2", 25, None, False), ("s2l3", "S2", 4, 4, False), ("s4", "S4", 3, None, False),
        ("d16", "16x8", 2, None, True)],
    3: [("s2", "S2", 25, None, False), ("u50", "50x8", 7, None, False)],
}
P1 = dataclasses.replace(twin.CONFIGS["S2"], cfl=8.0, E0=0.8)


def _raises(exc, call):
    try:
        call()
    except exc:
        return 1
    except Exception as e:  # noqa: BLE001
        return f"{type(e).__name__}: {e}"
    return 0


def _local_csr(csr, rb, re_):
    ip, ix, d = csr
    return d[ip[rb]:ip[re_]].copy(), ix[ip[rb]:ip[re_]].copy(), (ip[rb:re_ + 1] - ip[rb]).astype(np.int32)


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    out = {}

    def operator(name, dropin):
        p, csr, _, b = host_case(name)
        stride, period = direction(p)
        offs = vk.partition_rows(p.n, world, stride)
        rb, re_ = int(offs[rank]), int(offs[rank + 1])
        if dropin:
            A = vk.csr_matrix(_local_csr(csr, rb, re_), shape=(p.n, p.n), ctx=ctx, offsets=offs)
        else:
            A = vk.vlasov_operator(vparams(vk, p), ctx=ctx, offsets=offs)
        return p, A, b[rb:re_], rb, re_, stride, period

    # -- 4. refusals first: a rank left behind in one of their collectives would derail what follows
    p4 = twin.CONFIGS["S4"]
    sx, nx = direction(p4)
    A4 = vk.vlasov_operator(vparams(vk, p4), ctx=ctx, offsets=vk.partition_rows(p4.n, world, sx))
    out["ref_ylines"] = _raises(ValueError, lambda: vk.line_cyclic(A4, *direction(p4, "y"), 2, span=True))
    if nx // world < 3:   # two planes per rank
        out["ref_planes"] = _raises(ValueError, lambda: vk.line_cyclic(A4, sx, nx, 3, span=True))
    for args in ((sx, nx, 1), (sx, 2, 3), (0, nx, 3)):
        out[f"ref_args_{args[1]}_{args[2]}_{args[0] > 0}"] = _raises(ValueError, lambda a=args: vk.line_cyclic(A4, *a, span=True))

    for key, name, seg, serial, dropin in RANK_CASES[world]:
        p, A, bl, rb, re_, stride, period = operator(name, dropin)
        out[f"{key}_plain_refused"] = _raises(ValueError, lambda: vk.line_cyclic(A, stride, period, seg))
        with ctx.tuning(**({} if serial is None else {"linec_serial": serial})):
            M = vk.line_cyclic(A, stride, period, seg, span=True)
        out[f"{key}_rows"] = np.array([rb, re_])
        out[f"{key}_span"] = json.dumps(M.span_info)
        out[f"{key}_levels"] = np.array(M.info()["unknowns"])
        out[f"{key}_z"] = M @ bl
        out[f"{key}_z_again"] = int(np.array_equal(out[f"{key}_z"], M @ bl))
        for orth in ("dcgs2", "mgs"):
            x, info = vk.gmres(A, bl, rtol=1e-8, M=M, orth=orth)
            out.update({f"{key}_x_{orth}": x, f"{key}_info_{orth}": info, f"{key}_it_{orth}": vk.last_stats().inner_iters})
        x, info = vk.bicgstab(A, bl, rtol=1e-8, M=M, maxiter=500)
        st = vk.last_bicgstab_stats()
        out.update({f"{key}_x_bcg": x, f"{key}_info_bcg": info, f"{key}_it_bcg": st.iterations, f"{key}_half_bcg": st.half_step})
        if key == "s2":   # the other refusals, around a live spanning M
            out["ref_neumann"] = _raises(ValueError, lambda: vk.neumann(A, M, 2))
            lib, u, f = vk._abi.lib(), C.c_int(), np.empty(3 * max(re_ - rb, 1))
            fp = f.ctypes.data_as(C.c_void_p)
            for k, call in enumerate((lambda: lib.vtk_linejacobi_get_compact(M.handle, C.byref(u), None),
                                      lambda: lib.vtk_linejacobi_set_compact(M.handle, 0),
                                      lambda: lib.vtk_linejacobi_factors(M.handle, fp, vk._abi.PTR_HOST),
                                      lambda: lib.vtk_lineproduct_factors(M.handle, 0, fp, vk._abi.PTR_HOST))):
                out[f"ref_accessor{k}"] = int(call() == vk._abi.ERR_STATE)
        if key == "s2l3" and world == 2:   # -- 5. refresh after update_vlasov: the bits of a fresh M
            A.update_vlasov(vparams(vk, P1))
            lag = int(np.array_equal(M @ bl, out[f"{key}_z"]))
            with ctx.tuning(linec_serial=4):
                M.refresh()
                F = vk.line_cyclic(A, stride, period, seg, span=True)
            z1 = M @ bl
            out["rf_z"] = z1
            out["rf_flags"] = np.array([lag, int(np.array_equal(z1, F @ bl)), int(not np.array_equal(z1, out[f"{key}_z"])),
                                        int(M.values_epoch == 1)])
            F.close()
        if key == "d16" and world == 2:   # -- 5. a zero pivot planted on rank 1 only
            _, csr, _, _ = host_case(name)
            dl, ixl, ipl = _local_csr(csr, rb, re_)
            bad = dl.copy()
            if rank == 1:
                bad[ipl[0] + np.flatnonzero(ixl[ipl[0]:ipl[1]] == rb)[0]] = 0.0
            A.update_values(bad)
            msg = []
            sing = _raises(np.linalg.LinAlgError, lambda: M.refresh())
            try:
                M.refresh()
            except np.linalg.LinAlgError as e:
                msg.append(str(e))
            unusable = _raises(vk._abi.VtkError, lambda: M @ bl)
            A.update_values(dl)
            M.refresh()
            out["sg_flags"] = np.array([sing == 1, len(msg) == 1, unusable == 1, int(np.array_equal(M @ bl, out[f"{key}_z"]))]).astype(int)
            out["sg_msg"] = msg[0] if msg else ""
        M.close()
        A.close()
    A4.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), errors=np.array(hc.errors, dtype=object).astype(str),
             **{k: (np.asarray(v) if not isinstance(v, str) else v) for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


_RUNS = {}


def _run_ranks(world, tmp_path_factory):
    """One spawn per world and module run; its records are shared and left unchanged."""
    if world not in _RUNS:
        import torch.multiprocessing as mp
        d = tmp_path_factory.mktemp(f"span{world}")
        mp.spawn(_worker, args=(world, _free_port(), str(d)), nprocs=world, join=True)
        _RUNS[world] = [np.load(d / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    return world, _RUNS[world]


@pytest.fixture(scope="module", params=[2, 3], ids=["world2", "world3"])
def ranks(request, tmp_path_factory):
    return _run_ranks(request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return _run_ranks(2, tmp_path_factory)


def test_ranks_apply_and_solves(ranks):
    world, z = ranks
    for r in range(world):
        assert z[r]["errors"].size == 0, z[r]["errors"]
    for key, name, seg, serial, dropin in RANK_CASES[world]:
        p, csr, _, b = host_case(name)
        stride, period = direction(p)
        zz = np.zeros(p.n)
        xs = {k: np.zeros(p.n) for k in ("dcgs2", "mgs", "bcg")}
        lines = []
        for r in range(world):
            assert str(z[r][f"{key}_plain_refused"]) == "1", "the plain kind keeps refusing lines that span ranks"
            rb, re_ = (int(v) for v in z[r][f"{key}_rows"])
            si = json.loads(str(z[r][f"{key}_span"]))
            assert si == {"world": world, "rank": r, "first_line": rb // stride, "local_period": (re_ - rb) // stride,
                          "period": period, "spanning": True}, si
            assert int(z[r][f"{key}_levels"][0]) == si["local_period"]
            assert int(z[r][f"{key}_z_again"]) == 1
            lines.append(si["local_period"])
            zz[rb:re_] = z[r][f"{key}_z"]
            for k in xs:
                xs[k][rb:re_] = z[r][f"{key}_x_{k}"]
                assert int(z[r][f"{key}_info_{k}"]) == int(z[0][f"{key}_info_{k}"])
                assert int(z[r][f"{key}_it_{k}"]) == int(z[0][f"{key}_it_{k}"])
        print(f"world {world} {key}: lines per rank {lines}")
        assert sum(lines) == period and min(lines) >= 3
        if (world, key) == (3, "s2"):
            assert sorted(lines) == [21, 21, 22]   # (partition_rows gives 21 / 22 / 21)
        if (world, key) == (3, "u50"):
            assert len(set(lines)) > 1   # uneven
        check_apply(f"world {world} {key} span apply", zz, b, reference(name))
        for k in ("dcgs2", "mgs"):
            check_solve(xs[k], int(z[0][f"{key}_info_{k}"]), int(z[0][f"{key}_it_{k}"]), gmres_ref(name), csr, b)
        check_bicgstab(name, xs["bcg"], int(z[0][f"{key}_info_bcg"]), int(z[0][f"{key}_it_bcg"]), int(z[0][f"{key}_half_bcg"]))


def test_ranks_refusals(ranks):
    """Raised on every rank (the worker went on to its collectives afterwards)."""
    world, z = ranks
    keys = [k for k in z[0].files if k.startswith("ref_")]
    assert "ref_ylines" in keys and "ref_neumann" in keys and sum(k.startswith("ref_accessor") for k in keys) == 4
    assert ("ref_planes" in keys) == (world == 3)   # S4's six x-planes: two per rank at world 3
    for r in range(world):
        for k in keys:
            assert str(z[r][k]) == "1", (r, k, str(z[r][k]))


def test_ranks_refresh(two_ranks):
    world, z = two_ranks
    ip, ix, d = coracle.generate(P1)
    zz = np.zeros(P1.n)
    for r in range(world):
        assert z[r]["rf_flags"].tolist() == [1, 1, 1, 1], z[r]["rf_flags"]   # lagged until refresh; fresh M's bits; new values
        rb, re_ = (int(v) for v in z[r]["s2l3_rows"])
        zz[rb:re_] = z[r]["rf_z"]
        assert z[r]["sg_flags"].tolist() == [1, 1, 1, 1], (z[r]["sg_flags"], str(z[r]["sg_msg"]))
    check_apply("S2 refreshed across two ranks", zz, twin.rhs(P1.n), Reference(ip, ix, d, P1.n, *direction(P1)))
    # the failing rank names its row (the global one), the other names the rank
    rb1 = int(z[1]["d16_rows"][0])
    assert f"row {rb1} " in str(z[1]["sg_msg"]), str(z[1]["sg_msg"])
    assert "rank 1" in str(z[0]["sg_msg"]), str(z[0]["sg_msg"])


# ---- 4. the refusals on one rank ---------------------------------------------------------------------

def test_refusals_one_rank(ops, vk_lib):
    vk = vk_lib
    p = host_case("S4")[0]
    with pytest.raises(ValueError):
        vk.line_cyclic(ops["S4"], *direction(p, "y"), 2, span=True)   # n_global != stride * period
    p2 = host_case("S2")[0]
    stride, period = direction(p2)
    for args in ((stride, 2, 25), (stride, period, 1), (0, period, 25), (stride, period - 1, 25), (stride + 1, period, 25)):
        with pytest.raises(ValueError):
            vk.line_cyclic(ops["S2"], *args, span=True)
    M = vk.line_cyclic(ops["S2"], stride, period, 25, span=True)
    try:
        with pytest.raises(ValueError):
            vk.neumann(ops["S2"], M, 2)
        lib, h = vk._abi.lib(), ops["S2"].ctx.handle
        u, f = C.c_int(), np.empty(3 * p2.n)
        fp = f.ctypes.data_as(C.c_void_p)
        for call in (lambda: lib.vtk_linejacobi_get_compact(M.handle, C.byref(u), None),
                     lambda: lib.vtk_linejacobi_set_compact(M.handle, 0),
                     lambda: lib.vtk_linejacobi_factors(M.handle, fp, vk._abi.PTR_HOST),
                     lambda: lib.vtk_lineproduct_factors(M.handle, 0, fp, vk._abi.PTR_HOST)):
            with pytest.raises(vk._abi.VtkError) as e:
                vk._abi.check(call(), h)
            assert e.value.status == vk._abi.ERR_STATE
    finally:
        M.close()


# ---- 6. the vtsetup element --------------------------------------------------------------------------

def test_vtsetup_line_span(gpu, tmp_path):
    """preconditioner/line_span through the entry layer: one rank in this process, then run/gpus = 2
    (two rank processes on the host-staged transport), which the 2D operators need it for."""
    from vtsetup.config import SolverConfig
    from vtsetup.krylov_precondition import KrylovPrecondition
    cfg = SolverConfig.load(config="S2", preconditioner="line_cyclic", line_span=1, report=str(tmp_path / "r1.json"))
    step = KrylovPrecondition(cfg, ctx=gpu)
    r1 = step.main()
    x1 = np.asarray(step.x)
    assert r1["preconditioner"]["line_span"] == 1 and r1["solve"]["info"] == 0
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "vt-precondition_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, root]))
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, "-m", "vtsetup.krylov_precondition", "--config", "S2", "--preconditioner", "line_cyclic",
                          "--line-span", "--gpus", "2", "--comm", "host", "--report", str(tmp_path / "r2.json"),
                          "--x-out", str(tmp_path / "x2.npy")], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r2 = json.load(open(tmp_path / "r2.json"))
    x2 = np.load(tmp_path / "x2.npy")
    assert r2["ranks"] == 2 and r2["preconditioner"]["line_span"] == 1 and r2["solve"]["info"] == 0
    assert abs(r2["solve"]["inner_iters"] - r1["solve"]["inner_iters"]) <= 1
    assert np.max(np.abs(x2 - x1)) <= 1e-8 * np.max(np.abs(x1))
