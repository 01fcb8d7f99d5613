"""Band step without the diagonal read (tuning band_opt bit 6): on the band path
the block-Jacobi factors are the tridiagonal factors of A's current diagonal blocks, A = M + C, so
the band step and step 0 of its cycle form w = p + M^-1 (C p) instead of M^-1 (A p) and read no
diagonal table.

Different operations, the same operator: last-bit differences in w.  So the solves follow the
DCGS2 bars of tests/test_gpu_band.py against the same solve without the bit and against the C
oracle on the downloaded CSR -- the same info, inner iterations within +-1, ||x - x_ref|| /
||x_ref|| < 1e-9, true residual <= rtol ||b|| -- and are bit-identical from run to run.
Everything runs under band_long_rows=0 so that every bit is live at test sizes.
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

ND = 64


def _solve(vk, A, M, b, **kw):
    x, info = vk.gmres(A, b, rtol=kw.pop("rtol", 1e-8), M=M, **kw)
    return x, info, vk.last_stats()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The operator's CSR, BJ(8) inverse blocks and right-hand side of a named config (host, shared)."""
    p = twin.CONFIGS[name]
    ip, ix, d = coracle.generate(p)
    return p, (ip, ix, d), coracle.bj_setup(ip, ix, d, 8), coracle.rhs(p.n)


@functools.lru_cache(maxsize=None)
def _ref(name, restart=20, rtol=1e-8, x0seed=None):
    p, (ip, ix, d), inv, b = _case(name)
    x0 = None if x0seed is None else twin.rhs(p.n, seed=x0seed) * 1e-3
    return coracle.gmres(ip, ix, d, b, inv, x0=x0, rtol=rtol, restart=restart, maxiter=400)


def _bars(x, info, st, ref, csr, b, rtol=1e-8, tag=None):
    assert info == ref.info == 0 and st.band == 1, tag
    assert abs(st.inner_iters - ref.inner_iters) <= 1, (tag, st.inner_iters, ref.inner_iters)
    assert np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x) < 1e-9, tag
    assert np.linalg.norm(b - coracle.spmv(*csr, x)) <= rtol * np.linalg.norm(b), tag


def _vs_off(xa, ia, sa, x0_, i0, s0, tag=None):
    """Against the same solve with the bit off."""
    assert ia == i0 == 0 and s0.band == 1, tag
    assert abs(sa.inner_iters - s0.inner_iters) <= 1, (tag, sa.inner_iters, s0.inner_iters)
    assert np.linalg.norm(xa - x0_) / np.linalg.norm(x0_) < 1e-9, tag


def _op(vk, gpu, name):
    p = twin.CONFIGS[name]
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=gpu)
    return A, vk.block_jacobi(A, 8)


@pytest.mark.parametrize("name", ["S2", "C1"])
def test_nodiag_bars_and_repeat(vk_lib, gpu, name):
    p, csr, _, b = _case(name)
    ref = _ref(name)
    A, M = _op(vk_lib, gpu, name)
    with gpu.tuning(band_long_rows=0):
        for opt in (64, 67, 73, 127):
            with gpu.tuning(band_opt=opt & ~ND):
                x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=20)
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=20)
            _bars(xa, ia, sa, ref, csr, b, tag=opt)
            _vs_off(xa, ia, sa, x0_, i0, s0, tag=opt)
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, opt
    M.close()
    A.close()


@pytest.mark.parametrize("name", ["S2", "C1"])
def test_nodiag_bits_2_3_change_no_sum(vk_lib, gpu, name):
    """Bit 2 (a range's two parts on one XCD) and bit 3 (the LDS-DMA prefetch of J > 12, one row
    fewer with bit 6) change no operation: bit for bit the solve with bit 6 and without them."""
    p, csr, _, b = _case(name)
    A, M = _op(vk_lib, gpu, name)
    with gpu.tuning(band_long_rows=0):
        for opt in (0, 1, 2, 3):
            with gpu.tuning(band_opt=ND | opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20)
            assert ia == 0 and sa.band == 1, opt
            for extra in (4, 8, 12):
                with gpu.tuning(band_opt=ND | opt | extra):
                    xc, ic, sc = _solve(vk_lib, A, M, b, restart=20)
                assert ic == 0 and np.array_equal(xc, xa) and sc.inner_iters == sa.inner_iters, (opt, extra)
    M.close()
    A.close()


@pytest.mark.parametrize("restart", [2, 3, 5, 20])
def test_nodiag_restarts(vk_lib, gpu, restart):
    """Short restarts: every w feeds the next step and the cycle's x update with no averaging over
    a long basis (restart 2: step 0's kernel and band step j = 0 only)."""
    p, csr, _, b = _case("S2")
    ref = _ref("S2", restart=restart)
    A, M = _op(vk_lib, gpu, "S2")
    with gpu.tuning(band_long_rows=0):
        with gpu.tuning(band_opt=63):
            x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
        for opt in (64, 127):
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
            _bars(xa, ia, sa, ref, csr, b, tag=opt)
            _vs_off(xa, ia, sa, x0_, i0, s0, tag=opt)
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, opt
    M.close()
    A.close()


def test_nodiag_nonzero_x0_stops_on_odd_and_even_columns(vk_lib, gpu):
    p, csr, _, b = _case("C1")
    A, M = _op(vk_lib, gpu, "C1")
    x0 = twin.rhs(p.n, seed=0xB00) * 1e-3
    cols = []
    with gpu.tuning(band_long_rows=0):
        # (the oracle stops at columns 9, 18, 7, 16, 5; the GPU solve within one of them)
        for rtol in (1e-4, 1e-5, 1e-6, 1e-7, 1e-8):
            ref = _ref("C1", rtol=rtol, x0seed=0xB00)
            with gpu.tuning(band_opt=63):
                x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=20, rtol=rtol, x0=x0.copy())
            with gpu.tuning(band_opt=127):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20, rtol=rtol, x0=x0.copy())
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=20, rtol=rtol, x0=x0.copy())
            print(f"rtol {rtol:g}: inner {sa.inner_iters} (bit off {s0.inner_iters}, oracle {ref.inner_iters})")
            _bars(xa, ia, sa, ref, csr, b, rtol=rtol, tag=rtol)
            _vs_off(xa, ia, sa, x0_, i0, s0, tag=rtol)
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, rtol
            cols.append((sa.inner_iters - 1) % 20)   # the column whose step found the residual small
    assert any(c & 1 for c in cols) and any(not (c & 1) for c in cols), cols
    M.close()
    A.close()


def _shape_case(vk_lib, gpu, shape):
    A = vk_lib.vlasov_operator(vk_lib.vlasov_params(2, shape), ctx=gpu)
    assert A.line_band == shape[1]
    M = vk_lib.block_jacobi(A, 8)
    ip, ix, d = A.download()
    b = coracle.rhs(shape[0] * shape[1])
    ref = coracle.gmres(ip, ix, d, b, coracle.bj_setup(ip, ix, d, 8), rtol=1e-8, restart=20, maxiter=400)
    with gpu.tuning(band_long_rows=0):
        with gpu.tuning(band_opt=63):
            x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=20, maxiter=400)
        for opt in (64, 127):
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20, maxiter=400)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=20, maxiter=400)
            _bars(xa, ia, sa, ref, (ip, ix, d), b, tag=(shape, opt))
            _vs_off(xa, ia, sa, x0_, i0, s0, tag=(shape, opt))
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, (shape, opt)
    M.close()
    A.close()


@pytest.mark.parametrize("shape", [(48, 8), (40, 816), (24, 1000)])
def test_nodiag_line_lengths(vk_lib, gpu, shape):
    """L = 8: one block per line, C has no v term at all; L = 816: three parts of 272 rows, block
    edges on part edges and inside parts; L = 1000: five parts of 200 rows."""
    _shape_case(vk_lib, gpu, shape)


@pytest.mark.parametrize("Nv", [32, 800])
@pytest.mark.parametrize("Nx", [3, 4, 7])
def test_nodiag_few_lines(vk_lib, gpu, Nx, Nv):
    """Operators of 3, 4 and 7 lines: the wrap lines (first and last line of the rank) and with them
    every canonical order of a row's entries; at 3 lines one range whose halo lines are its own."""
    _shape_case(vk_lib, gpu, (Nx, Nv))


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
    offs = vk.partition_rows(p.n, world, p.shape[-1])
    rb, re_ = int(offs[rank]), int(offs[rank + 1])
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=ctx, offsets=offs)
    M = vk.block_jacobi(A, 8)
    b = coracle.rhs(p.n)[rb:re_]
    out = {}
    ctx.set_tuning("band_long_rows", 0)
    for tag, opt in (("a", 127), ("b", 127), ("r", 63)):
        ctx.set_tuning("band_opt", opt)
        x, info = vk.gmres(A, b, rtol=1e-8, M=M, orth="dcgs2")
        st = vk.last_stats()
        out.update({f"x_{tag}": x, f"info_{tag}": info, f"iters_{tag}": st.inner_iters, f"band_{tag}": st.band})
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), commlog=json.dumps(hc.log), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("S2", 2), ("S2", 3), ("C1", 2), ("C1", 3)])
def test_nodiag_across_ranks(tmp_path, case, world):
    """Host-staged ranks sharing the GPU (the ghost-line variant): blocks never straddle ranks and
    the halo columns are entries of C, so the identity holds rank by rank."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(world, _free_port(), case, str(tmp_path)), nprocs=world, join=True)
    p, csr, _, b = _case(case)
    ref = _ref(case)
    z = [np.load(tmp_path / f"rank{r}.npz", allow_pickle=False) for r in range(world)]
    xs = {t: np.zeros(p.n) for t in "abr"}
    for r in range(world):
        assert z[r]["errors"].size == 0, z[r]["errors"]
        for t in "abr":
            assert int(z[r][f"info_{t}"]) == 0 and int(z[r][f"band_{t}"]) == 1, (r, t)
            assert int(z[r][f"iters_{t}"]) == int(z[0][f"iters_{t}"]), (r, t)
            xs[t][int(z[r]["rb"]):int(z[r]["re"])] = z[r][f"x_{t}"]
    it = {t: int(z[0][f"iters_{t}"]) for t in "abr"}
    assert abs(it["a"] - ref.inner_iters) <= 1 and abs(it["a"] - it["r"]) <= 1, (it, ref.inner_iters)
    assert np.linalg.norm(xs["a"] - ref.x) / np.linalg.norm(ref.x) < 1e-9
    assert np.linalg.norm(xs["a"] - xs["r"]) / np.linalg.norm(xs["r"]) < 1e-9
    assert np.linalg.norm(b - coracle.spmv(*csr, xs["a"])) <= 1e-8 * np.linalg.norm(b)
    assert it["a"] == it["b"] and np.array_equal(xs["a"], xs["b"]), "not bit-identical on repeat"
    from vtkrylov.comm import check_sequences
    check_sequences([json.loads(str(q["commlog"])) for q in z])


P1 = dict(cfl=8.0, E0=0.8, nu=0.1)


def _vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


@pytest.mark.parametrize("how", ["update_vlasov", "update_values"])
def test_nodiag_guard_lagged_preconditioner(vk_lib, gpu, how):
    """w = p + M^-1 (A - M) p is M^-1 A p only for the M of A's current values.  A preconditioner
    that was not refreshed after a value update must not reach the band step: the solve leaves the
    band path and applies the lagged inverse to the new operator; the refresh brings the band back."""
    p0 = twin.CONFIGS["S2"]
    p1 = dataclasses.replace(p0, **P1)
    csr0, csr1 = coracle.generate(p0), coracle.generate(p1)
    inv0, inv1 = coracle.bj_setup(*csr0, 8), coracle.bj_setup(*csr1, 8)
    b = twin.rhs(p0.n)
    A = vk_lib.vlasov_operator(_vparams(vk_lib, p0), ctx=gpu)
    M = vk_lib.block_jacobi(A, 8)
    with gpu.tuning(band_long_rows=0, band_opt=127):
        x, info, st = _solve(vk_lib, A, M, b, maxiter=100)
        _bars(x, info, st, coracle.gmres(*csr0, b, inv0, rtol=1e-8), csr0, b, tag="before")
        if how == "update_vlasov":
            A.update_vlasov(_vparams(vk_lib, p1))
        else:
            A.update_values(csr1[2])
        assert (A.values_epoch, M.values_epoch) == (1, 0)
        x, info, st = _solve(vk_lib, A, M, b, maxiter=100)
        ref = coracle.gmres(*csr1, b, inv0, rtol=1e-8)   # the new values, the lagged inverse
        assert st.band == 0, "a lagged M reached the band step"
        assert info == ref.info == 0 and abs(st.inner_iters - ref.inner_iters) <= 1, (st.inner_iters, ref.inner_iters)
        assert np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x) < 1e-9
        assert np.linalg.norm(b - coracle.spmv(*csr1, x)) <= 1e-8 * np.linalg.norm(b)
        M.refresh()
        x, info, st = _solve(vk_lib, A, M, b, maxiter=100)
        _bars(x, info, st, coracle.gmres(*csr1, b, inv1, rtol=1e-8), csr1, b, tag="refreshed")
    M.close()
    A.close()


def test_nodiag_profile_bytes(vk_lib, gpu):
    """The byte model follows the kernel: every band step launch books exactly 8 n bytes fewer with
    the bit (the diagonal table's row), and step 0 of the cycle likewise."""
    p, csr, _, b = _case("S2")
    A, M = _op(vk_lib, gpu, "S2")
    per = {}
    with gpu.tuning(band_long_rows=0, prof_perj=1):
        for opt in (63, 127):
            with gpu.tuning(band_opt=opt):
                gpu.profile(True)
                x, info, st = _solve(vk_lib, A, M, b, restart=20)
                pr = gpu.profile_read()
                gpu.profile(False)
            assert info == 0 and st.band == 1
            per[opt] = {k: e["bytes"] / e["launches"] for k, e in pr.items()
                        if k.startswith("band_step") or k == "spmv_bj_dc"}
    assert set(per[63]) == set(per[127]) and "spmv_bj_dc" in per[63] and "band_step_j00" in per[63], per
    for k in per[63]:
        assert per[63][k] - per[127][k] == 8.0 * p.n, (k, per[63][k], per[127][k])
    M.close()
    A.close()
