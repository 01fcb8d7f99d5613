"""vtkrylov.bicgstab across ranks on the single-GPU test box: W processes share cuda:0 and talk
through the host-staged communicator (vtk_comm_init_host over gloo), as tests/test_gpu_multirank.py
does for GMRES.  The reference is the one-rank NumPy twin of scipy.sparse.linalg.bicgstab; the bars
are the one-rank BiCGStab bars (tests/test_gpu_bicgstab.py), whose premise for rank-partitioned sums
tests/test_bicgstab_ranks_host.py checks on the CPU.  Two line-preconditioned cases are sharp and are
held to equal counts, equal exits and 1e-9.

One spawn runs all the solves of its case; every solve passes maxiter <= 500; the process group has
a 60 s timeout, so a mismatched collective raises instead of hanging.  The parity worker also runs
the truncated solves of tests/test_gpu_bicgstab_steps.py (its ``steps`` plan).
"""
import functools
import json
import os
import socket

import numpy as np
import pytest

from oracle import twin
from test_bicgstab_host import BREAKDOWNS, bicgstab_twin
from test_bicgstab_ranks_host import LINE_SEG, MAXIT, SHARP, host_system, ref, slab_offsets, slab_unit
from test_gpu_bicgstab import line_geometry, true_residual, within_bars
from test_gpu_bicgstab import ref as ref_one_rank

pytestmark = pytest.mark.gpu

LOOKAHEAD = 3   # iterations the host enqueues ahead of the device (vtk_driver.hpp)
KINDS = [("none", "auto"), ("bj8", "auto"), ("bj8", "inverse"), ("bj16", "auto"), ("line", "auto")]
RTOLS = [1e-5, 1e-8]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _join(rank, world, port):
    import datetime
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    import vtkrylov as vk
    ctx = vk.Context(0)
    return dist, vk, ctx, ctx.comm_init_host(rank, world)


def _leave(dist):
    dist.barrier()
    dist.destroy_process_group()


def _operator(vk, ctx, name, world, layout=None, even=True):
    """even: equal slabs (slab_offsets); else the library's partition in whole lines / planes, for a
    world that does not divide them."""
    p = twin.CONFIGS[name]
    offs = slab_offsets(name, world) if even else vk.partition_rows(p.n, world, slab_unit(p))
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=ctx, offsets=offs)
    if layout:
        A.set_layout(layout)
    return A, int(offs[ctx.rank]), int(offs[ctx.rank + 1])


def _prec(vk, A, name, world, kind, mode):
    if kind == "none":
        return None
    if kind.startswith("bj"):
        return vk.block_jacobi(A, int(kind[2:]), mode)
    return vk.line_jacobi(A, slab_unit(twin.CONFIGS[name]), LINE_SEG[(name, world)])


def _stats(st):
    return dict(iterations=int(st.iterations), half_step=int(st.half_step), rnorm=float(st.rnorm).hex(),
                bnorm=float(st.bnorm).hex(), atol_eff=float(st.atol_eff).hex())


def reference(name, kind, rtol, seg=0):
    """The np.dot twin's (x, info, iterations, half_step): the one-rank GPU tests' cached run where
    the preconditioner is the same (always, but for a line segment other than theirs)."""
    if kind != "line" or seg == line_geometry(name)[1]:
        return ref_one_rank(name, kind, rtol)
    return ref(name, kind, rtol, seg)


def _st(m):
    import types
    return types.SimpleNamespace(iterations=m["iterations"], half_step=m["half_step"])


def _kinds(name):
    return [k for k in KINDS if name != "C1" or k in (("bj8", "auto"), ("line", "auto"))]


# ---- 1, 5. parity and the collective sequence of the clean solves ------------------------------

def _parity_worker(rank, world, port, name, layout, outdir, steps=None):
    """steps None: every kind of the case to both tolerances.  steps = ((kind, mode, (k, ...)), ...):
    the truncated runs rtol = atol = 0, maxiter = k of tests/test_gpu_bicgstab_steps.py, on the
    library's own partition (any world)."""
    dist, vk, ctx, hc = _join(rank, world, port)
    A, rb, re_ = _operator(vk, ctx, name, world, layout, even=steps is None)
    b = twin.rhs(twin.CONFIGS[name].n)[rb:re_]
    out, xs = [], {}
    if steps is None:
        plan = [(kind, mode, [dict(rtol=rtol, maxiter=MAXIT) for rtol in RTOLS]) for kind, mode in _kinds(name)]
    else:
        plan = [(kind, mode, [dict(rtol=0.0, atol=0.0, maxiter=k) for k in ks]) for kind, mode, ks in steps]
    for kind, mode, solves in plan:
        M = _prec(vk, A, name, world, kind, mode)
        if mode != "auto":
            assert M.mode == mode, M.mode
        for kw in solves:
            op0 = len(hc.log)
            x, info = vk.bicgstab(A, b, M=M, **kw)
            halo = sum(1 for o in hc.log[op0:] if o[0] == "alltoallv")
            xs[f"x{len(out)}"] = x
            out.append(dict(kind=kind, mode=mode, rtol=kw["rtol"], maxiter=kw["maxiter"], info=int(info), halo_ops=halo,
                            ops=len(hc.log) - op0, **_stats(vk.last_bicgstab_stats())))
        if M is not None:
            M.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_, meta=json.dumps(out), commlog=json.dumps(hc.log),
             errors=np.array(hc.errors, dtype=object).astype(str), **xs)
    _leave(dist)


PARITY = [("S2", 2, "csr"), ("S2", 2, "sell"), ("S2", 4, "csr"), ("S2", 4, "sell"), ("S4", 3, None), ("S4F", 2, None),
          ("C1", 2, None)]


@functools.lru_cache(maxsize=None)
def _parity_run(name, world, layout, steps=None):
    """One spawn per case, shared by the tests below: (per-rank meta lists, gathered x per solve,
    per-rank communicator logs).  steps: _parity_worker's."""
    import tempfile

    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_parity_worker, args=(world, _free_port(), name, layout, d, steps), nprocs=world, join=True)
        z = [np.load(os.path.join(d, f"rank{r}.npz"), allow_pickle=False) for r in range(world)]
        for q in z:
            assert q["errors"].size == 0, q["errors"]
        meta = [json.loads(str(q["meta"])) for q in z]
        logs = [json.loads(str(q["commlog"])) for q in z]
        xs = []
        for i in range(len(meta[0])):
            x = np.zeros(twin.CONFIGS[name].n)
            for q in z:
                x[int(q["rb"]):int(q["re"])] = q[f"x{i}"]
            xs.append(x)
    return meta, xs, logs


@pytest.mark.parametrize("name,world,layout", PARITY)
def test_parity_across_ranks(name, world, layout):
    meta, xs, _ = _parity_run(name, world, layout)
    p, csr, _, b = host_system(name)
    assert len(meta[0]) == len(_kinds(name)) * len(RTOLS)
    for i, m in enumerate(meta[0]):
        kind, rtol = m["kind"], m["rtol"]
        print(f"-- {name} world {world} {layout} {kind}/{m['mode']} rtol {rtol}")
        for other in meta[1:]:   # the same bits on every rank
            for key in ("info", "iterations", "half_step", "rnorm", "bnorm", "atol_eff"):
                assert other[i][key] == m[key], (key, other[i][key], m[key])
        seg = LINE_SEG[(name, world)] if kind == "line" else 0
        r = reference(name, kind, rtol, seg)
        within_bars(xs[i], m["info"], _st(m), r, csr, b, rtol)
        atol_eff, rnorm = float.fromhex(m["atol_eff"]), float.fromhex(m["rnorm"])
        assert float.fromhex(m["bnorm"]) == pytest.approx(np.linalg.norm(b), rel=1e-12)
        assert abs(rnorm - true_residual(csr, b, xs[i])) <= 1e-6 * atol_eff
        if kind == "line" and (name, world, rtol) in SHARP:
            assert (r[2], r[3]) == SHARP[(name, world, rtol)]
            assert (m["iterations"], m["half_step"]) == (r[2], r[3])
            rel = np.linalg.norm(xs[i] - r[0]) / np.linalg.norm(r[0])
            print(f"sharp: x_rel {rel:.3e}")
            assert rel <= 1e-9, rel


@pytest.mark.parametrize("name,world,layout", PARITY)
def test_collective_sequence(name, world, layout):
    """Every rank issued the sequence RCCL could run, and a solve exchanges its halo at most twice
    per enqueued iteration (the iterations that count, the look-ahead, the one that stopped) plus
    the initial and the true residual."""
    from vtkrylov.comm import check_sequences
    meta, _, logs = _parity_run(name, world, layout)
    check_sequences(logs)
    for ms in meta:
        for i, m in enumerate(ms):
            assert m["halo_ops"] <= 2 * (m["iterations"] + LOOKAHEAD + 1) + 2, m
            assert m["ops"] == meta[0][i]["ops"]


# ---- 2. the host decisions before the loop are global -------------------------------------------

def _decisions_worker(rank, world, port, outdir):
    dist, vk, ctx, hc = _join(rank, world, port)
    A, rb, re_ = _operator(vk, ctx, "S2", world)
    n = twin.CONFIGS["S2"].n
    M = vk.block_jacobi(A, 8)
    b = twin.rhs(n)
    out, xs = [], {}

    def solve(bv, x0, **kw):
        x, info = vk.bicgstab(A, bv[rb:re_], None if x0 is None else x0[rb:re_], M=M, **kw)
        xs[f"x{len(out)}"] = x
        out.append(dict(info=int(info), **_stats(vk.last_bicgstab_stats())))
    bz = b.copy()
    bz[:n // 2] = 0.0                                   # 0: b zero on rank 0's slab only
    solve(bz, None, rtol=1e-8, maxiter=MAXIT)
    x0 = np.zeros(n)
    x0[n // 2:] = twin.rhs(n, seed=3)[n // 2:]          # 1: x0 non-zero on rank 1's slab only
    solve(b, x0, rtol=1e-8, maxiter=MAXIT)
    solve(np.zeros(n), twin.rhs(n, seed=3), rtol=1e-8, maxiter=MAXIT)   # 2: b = 0 everywhere
    solve(b, None, rtol=1e-8, maxiter=3)                # 3: truncated
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_, meta=json.dumps(out), commlog=json.dumps(hc.log),
             errors=np.array(hc.errors, dtype=object).astype(str), **xs)
    _leave(dist)


def _gather(tmp_path, world, n):
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    for q in z:
        assert q["errors"].size == 0, q["errors"]
    meta = [json.loads(str(q["meta"])) for q in z]
    xs = []
    for i in range(len(meta[0])):
        x = np.zeros(n)
        for q in z:
            x[int(q["rb"]):int(q["re"])] = q[f"x{i}"]
        xs.append(x)
    return z, meta, xs


def test_host_decisions_are_global(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_decisions_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    p, csr, _, b = host_system("S2")
    z, meta, xs = _gather(tmp_path, 2, p.n)
    assert meta[0] == meta[1]   # info and every statistic, bit for bit
    st = _st
    m = meta[0]
    # b zero on rank 0's slab: locally ||b|| = 0 there, globally not -- the solve runs
    bz = b.copy()
    bz[:p.n // 2] = 0.0
    within_bars(xs[0], m[0]["info"], st(m[0]), ref("S2", "bj8", 1e-8, b_zero_to=p.n // 2), csr, bz, 1e-8)
    assert m[0]["iterations"] > 0
    # x0 non-zero on rank 1's slab only: both ranks take r = b - A x0
    within_bars(xs[1], m[1]["info"], st(m[1]), ref("S2", "bj8", 1e-8, x0_seed=3), csr, b, 1e-8)
    # b = 0 everywhere
    assert (m[2]["info"], m[2]["iterations"]) == (0, 0) and not xs[2].any()
    # maxiter = 3
    xr, infor, itr, _ = ref("S2", "bj8", 1e-8, maxiter=3)
    assert infor == 3 and itr == 3
    assert (m[3]["info"], m[3]["iterations"], m[3]["half_step"]) == (3, 3, 0)
    rel = np.linalg.norm(xs[3] - xr) / np.linalg.norm(xr)
    print(f"truncated: x_rel {rel:.3e}")
    assert rel <= 1e-9, rel
    from vtkrylov.comm import check_sequences
    check_sequences([json.loads(str(q["commlog"])) for q in z])


# ---- 3. exact breakdowns ------------------------------------------------------------------------

COPIES = 64
SPLITS = [3 * (COPIES // 2), 3 * (COPIES // 2) + 1]   # at a block boundary, inside a block


def _breakdown_system(case):
    import scipy.sparse as sp
    A3, b3, want = BREAKDOWNS[case]
    H = sp.kron(sp.identity(COPIES), sp.csr_matrix(np.array(A3, dtype=np.float64)), format="csr")
    return H, np.tile(np.array(b3, dtype=np.float64), COPIES), want


def _breakdown_worker(rank, world, port, outdir):
    dist, vk, ctx, hc = _join(rank, world, port)
    out, xs = [], {}
    for case in range(len(BREAKDOWNS)):
        H, b, _ = _breakdown_system(case)
        n = H.shape[0]
        for cut in SPLITS:
            offs = np.array([0, cut, n], dtype=np.int64)
            rb, re_ = int(offs[rank]), int(offs[rank + 1])
            Hl = H[rb:re_]
            A = vk.csr_matrix((Hl.data, Hl.indices, Hl.indptr), shape=(n, n), ctx=ctx, offsets=offs)
            x, info = vk.bicgstab(A, b[rb:re_], rtol=1e-12, maxiter=MAXIT)
            xs[f"x{len(out)}"] = x
            out.append(dict(case=case, cut=cut, rb=rb, re=re_, info=int(info), **_stats(vk.last_bicgstab_stats())))
            A.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), meta=json.dumps(out), commlog=json.dumps(hc.log),
             errors=np.array(hc.errors, dtype=object).astype(str), **xs)
    _leave(dist)


def test_exact_breakdowns_across_ranks(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_breakdown_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(2)]
    meta = [json.loads(str(q["meta"])) for q in z]
    assert len(meta[0]) == len(BREAKDOWNS) * len(SPLITS)
    for i, m in enumerate(meta[0]):
        H, b, (want_info, want_its) = _breakdown_system(m["case"])
        xr, infor, itr, _ = bicgstab_twin(H, b, rtol=1e-12, maxiter=MAXIT)
        assert (infor, itr) == (want_info, want_its)
        x = np.zeros(H.shape[0])
        for r in range(2):
            q = meta[r][i]
            assert z[r]["errors"].size == 0, z[r]["errors"]
            assert (q["info"], q["iterations"], q["half_step"]) == (want_info, want_its, 0), (r, q)
            x[q["rb"]:q["re"]] = z[r][f"x{i}"]
        assert np.array_equal(x, xr), (m, np.abs(x - xr).max())   # every sum is exact in any order
    from vtkrylov.comm import check_sequences
    check_sequences([json.loads(str(q["commlog"])) for q in z])


# ---- 4. failure containment ---------------------------------------------------------------------

def _fail_worker(rank, world, port, name, fail_rank, fail_step, outdir):
    import time
    dist, vk, ctx, hc = _join(rank, world, port)
    A, rb, re_ = _operator(vk, ctx, name, world)
    M = vk.block_jacobi(A, 8)
    b = twin.rhs(twin.CONFIGS[name].n)[rb:re_]
    if rank == fail_rank:
        ctx.set_tuning("fail_step", fail_step)
    op0 = len(hc.log)
    t = time.perf_counter()
    status, msg = 0, ""
    try:
        vk.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    except vk._abi.VtkError as e:
        status, msg = e.status, str(e)
    elapsed = time.perf_counter() - t
    ops_failed = len(hc.log) - op0
    ctx.set_tuning("fail_step", -1)
    x2, info2 = vk.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_, status=status, msg=msg, elapsed=elapsed,
             ops_failed=ops_failed, x0=x2, meta=json.dumps([dict(info=int(info2), **_stats(vk.last_bicgstab_stats()))]),
             commlog=json.dumps(hc.log), errors=np.array(hc.errors, dtype=object).astype(str))
    _leave(dist)


@pytest.mark.parametrize("name,world,fail_rank,fail_step", [("S2", 2, 1, 3), ("S4", 3, 0, 0)])
def test_peer_failure_is_contained(tmp_path, name, world, fail_rank, fail_step):
    """A rank whose launch is refused mid-solve votes the failure into the next all-reduce and keeps
    issuing the same launches and collectives: every rank leaves at the same point, the failing one
    with its own error and the others with ERR_PEER, and the communicator stays usable."""
    import torch.multiprocessing as mp

    import vtkrylov as vk
    mp.spawn(_fail_worker, args=(world, _free_port(), name, fail_rank, fail_step, str(tmp_path)), nprocs=world, join=True)
    p, csr, _, b = host_system(name)
    z, meta, xs = _gather(tmp_path, world, p.n)
    for r in range(world):
        st, msg = int(z[r]["status"]), str(z[r]["msg"])
        if r == fail_rank:
            assert st == vk._abi.ERR_HIP and "injected failure" in msg, (st, msg)
        else:
            assert st == vk._abi.ERR_PEER and "peer rank failed" in msg, (st, msg)
        assert float(z[r]["elapsed"]) < 30.0
        assert meta[r] == meta[0]
    assert len({int(q["ops_failed"]) for q in z}) == 1, [int(q["ops_failed"]) for q in z]
    m = meta[0][0]
    within_bars(xs[0], m["info"], _st(m), reference(name, "bj8", 1e-8), csr, b, 1e-8)
    from vtkrylov.comm import check_sequences
    check_sequences([json.loads(str(q["commlog"])) for q in z])
