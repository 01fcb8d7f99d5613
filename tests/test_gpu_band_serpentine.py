"""Band step walk direction by step parity (tuning band_opt bit 5): odd steps walk
every line range the other way round, on top of bit 4's range parity, so that a step begins with
the lines the previous step touched last (Infinity Cache reuse).

A reversed walk sums a range's lines in the other order: last-bit differences in the dots, every
per-row quantity (v_j, p_{j+1}, w, the x update) the same operations.  So the solves follow the
DCGS2 bars of tests/test_gpu_band.py -- info 0, the band path taken, inner iterations within +-1
of the same solve without the bit and of the C oracle, ||x - x_ref|| / ||x_ref|| < 1e-9, true
residual <= rtol ||b|| -- and are bit-identical from run to run.  Everything runs under
band_long_rows=0 so that every bit is live at test sizes.
"""
import functools
import os
import socket

import numpy as np
import pytest

from oracle import coracle, twin

pytestmark = pytest.mark.gpu

SERP = 32


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


def _op(vk, gpu, name):
    p = twin.CONFIGS[name]
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=gpu)
    return A, vk.block_jacobi(A, 8)


@pytest.mark.parametrize("name", ["S2", "C1"])
def test_serpentine_bars_and_repeat(vk_lib, gpu, name):
    p, csr, _, b = _case(name)
    ref = _ref(name)
    A, M = _op(vk_lib, gpu, name)
    with gpu.tuning(band_long_rows=0):
        for opt in (32, 33, 34, 35, 63):
            with gpu.tuning(band_opt=opt & ~SERP):
                x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=20)
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=20)
            assert i0 == 0 and s0.band == 1, opt
            _bars(xa, ia, sa, ref, csr, b, tag=opt)
            assert abs(sa.inner_iters - s0.inner_iters) <= 1, opt
            assert np.linalg.norm(xa - x0_) / np.linalg.norm(x0_) < 1e-9, opt
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, opt
    M.close()
    A.close()


@pytest.mark.parametrize("name", ["S2", "C1"])
def test_serpentine_bits_2_3_change_no_sum(vk_lib, gpu, name):
    """Bit 2 (a range's two parts on one XCD) and bit 3 (the LDS-DMA prefetch of J > 12) move no
    line in the walk: bit for bit the solve without them, reversed steps included."""
    p, csr, _, b = _case(name)
    A, M = _op(vk_lib, gpu, name)
    with gpu.tuning(band_long_rows=0):
        for opt in (0, 1, 2, 3):
            with gpu.tuning(band_opt=SERP | opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20)
            assert ia == 0 and sa.band == 1, opt
            for extra in (4, 8, 12):
                with gpu.tuning(band_opt=SERP | opt | extra):
                    xc, ic, sc = _solve(vk_lib, A, M, b, restart=20)
                assert ic == 0 and np.array_equal(xc, xa) and sc.inner_iters == sa.inner_iters, (opt, extra)
    M.close()
    A.close()


@pytest.mark.parametrize("restart", [2, 3, 5])
def test_serpentine_short_restarts(vk_lib, gpu, restart):
    """Restart 2: band step j = 0 only (never reversed); 3: j = 0, 1; 5: both parities and a
    restart boundary after a reversed step."""
    p, csr, _, b = _case("S2")
    ref = _ref("S2", restart=restart)
    A, M = _op(vk_lib, gpu, "S2")
    with gpu.tuning(band_long_rows=0):
        with gpu.tuning(band_opt=31):
            x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
        assert i0 == 0 and s0.band == 1
        for opt in (32, 63):
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=restart, maxiter=400)
            _bars(xa, ia, sa, ref, csr, b, tag=opt)
            assert abs(sa.inner_iters - s0.inner_iters) <= 1, opt
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, opt
    M.close()
    A.close()


@pytest.mark.parametrize("Nv", [32, 800])
@pytest.mark.parametrize("Nx", [3, 4, 7])
def test_serpentine_few_lines_per_range(vk_lib, gpu, Nx, Nv):
    """Ranges of a few lines: a walk's first and last iterations are the x-halo lines, so most of
    a reversed walk is its two ends (at 3 lines one range whose halo lines are its own)."""
    A = vk_lib.vlasov_operator(vk_lib.vlasov_params(2, (Nx, Nv)), ctx=gpu)
    M = vk_lib.block_jacobi(A, 8)
    ip, ix, d = A.download()
    b = coracle.rhs(Nx * Nv)
    ref = coracle.gmres(ip, ix, d, b, coracle.bj_setup(ip, ix, d, 8), rtol=1e-8, restart=20, maxiter=400)
    with gpu.tuning(band_long_rows=0):
        with gpu.tuning(band_opt=31):
            x0_, i0, s0 = _solve(vk_lib, A, M, b, restart=20)
        assert i0 == 0 and s0.band == 1
        for opt in (32, 63):
            with gpu.tuning(band_opt=opt):
                xa, ia, sa = _solve(vk_lib, A, M, b, restart=20)
                xb, ib, sb = _solve(vk_lib, A, M, b, restart=20)
            _bars(xa, ia, sa, ref, (ip, ix, d), b, tag=opt)
            assert abs(sa.inner_iters - s0.inner_iters) <= 1, opt
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, opt
    M.close()
    A.close()


def test_serpentine_stops_inside_reversed_step(vk_lib, gpu):
    """Solves that stop at an odd and at an even column: the inlined x update and the early commit
    run after (or, as the x-update launch of the band kernel, in place of) a reversed step."""
    p, csr, _, b = _case("C1")
    A, M = _op(vk_lib, gpu, "C1")
    x0 = twin.rhs(p.n, seed=0xB00) * 1e-3
    cols = []
    with gpu.tuning(band_long_rows=0, band_opt=63):
        # (the oracle stops at columns 9, 18, 7, 16, 5; the GPU solve within one of them)
        for rtol in (1e-4, 1e-5, 1e-6, 1e-7, 1e-8):
            ref = _ref("C1", rtol=rtol, x0seed=0xB00)
            xa, ia, sa = _solve(vk_lib, A, M, b, restart=20, rtol=rtol, x0=x0.copy())
            xb, ib, sb = _solve(vk_lib, A, M, b, restart=20, rtol=rtol, x0=x0.copy())
            print(f"rtol {rtol:g}: inner {sa.inner_iters} (oracle {ref.inner_iters})")
            _bars(xa, ia, sa, ref, csr, b, rtol=rtol, tag=rtol)
            assert ib == 0 and np.array_equal(xa, xb) and sa.inner_iters == sb.inner_iters, rtol
            cols.append((sa.inner_iters - 1) % 20)   # the column whose step found the residual small
    assert any(c & 1 for c in cols) and any(not (c & 1) for c in cols), cols
    M.close()
    A.close()


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
    for tag, opt in (("a", 63), ("b", 63), ("r", 31)):
        ctx.set_tuning("band_opt", opt)
        x, info = vk.gmres(A, b, rtol=1e-8, M=M, orth="dcgs2")
        st = vk.last_stats()
        out.update({f"x_{tag}": x, f"info_{tag}": info, f"iters_{tag}": st.inner_iters, f"band_{tag}": st.band})
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), rb=rb, re=re_,
             errors=np.array(hc.errors, dtype=object).astype(str), **out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case,world", [("S2", 2), ("S2", 3), ("C1", 2), ("C1", 3)])
def test_serpentine_across_ranks(tmp_path, case, world):
    """Host-staged ranks sharing the GPU: a rank's first / last range reads its x-halo line from
    the ghost buffer at whichever end of the walk it now comes (with three ranks the last range's
    parity is odd on one of them)."""
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
