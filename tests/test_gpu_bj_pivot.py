"""Block Jacobi where the Vlasov operators never go (inputs: oracle/cases.py, pinned on the CPU by
test_oracle_cases.py):

* partial pivoting in the exact setups -- k_bj_setup<VT, BS> (lane per row, shuffle-butterfly
  argmax; bs 1 .. 32) and k_bj_setup_generic (every other bs) -- on blocks with zero diagonals,
  integer entries (exact |a| ties: the rule "first row of largest |a|"), a padded last block and
  a non-canonical row, f64 and f32 values: inverse and apply bit-identical to the oracle;
* exactly singular blocks (zero block column / row, also in the padded block): LinAlgError;
* the tridiagonal-factor check of k_bj_tri_setup on tridiagonal blocks: factors accurate
  (d0 = 1e-4) -> the tridiagonal apply is used; Thomas without pivoting inaccurate (d0 = 1e-8)
  or its leading pivot zero (d0 = 0) -> rejected, the inverse apply is used;
* w = M^-1 (A x) of vtk_precond_matvec (the SpMV with the block-Jacobi epilogue for power-of-two
  bs <= 32, SpMV then apply otherwise) in every layout against the oracle's bj_apply(spmv(x)).
"""
import numpy as np
import pytest

from oracle import cases, coracle, twin

pytestmark = pytest.mark.gpu

PIVOT_BS = [1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 33, 63, 64]
FUSED_BS = [1, 2, 4, 8, 16, 32]      # the SpMV kernels' BJ epilogue
SPLIT_BS = [3, 7, 33, 64]            # SpMV, then k_bj_apply
LAYOUTS = ["sell", "sell32", "csr"]


def _blocks_close(got, ref, bs, tol):
    """test_gpu_bj_mfma._blocks_close."""
    g = got.reshape(-1, bs, bs)
    r = ref.reshape(-1, bs, bs)
    scale = np.abs(r).max(axis=(1, 2), keepdims=True)
    err = np.abs(g - r) / scale
    assert err.max() <= tol, err.max()


def _op(vk, gpu, csr):
    ip, ix, d = csr
    n = ip.shape[0] - 1
    return vk.csr_matrix((d, ix, ip), shape=(n, n), ctx=gpu), n


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("ints", [False, True], ids=["normal", "ints"])
@pytest.mark.parametrize("bs", PIVOT_BS)
def test_exact_setup_pivoting_bitexact(gpu, vk_lib, bs, ints, fp32):
    csr = cases.pivot_blocks(bs, 0, ints, fp32)
    A, n = _op(vk_lib, gpu, csr)
    assert A.fp32 == fp32
    M = vk_lib.block_jacobi(A, bs, mode="inverse", setup="exact")
    assert M.mode == "inverse"
    inv = coracle.bj_setup(*csr, bs)
    got = M.inverse()
    assert np.array_equal(got, inv), np.abs(got - inv).max()
    b = twin.rhs(n)
    assert np.array_equal(M @ b, coracle.bj_apply(inv, b))
    M.close()
    A.close()


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("bs", [16, 32])
def test_mfma_setup_integer_ties(gpu, vk_lib, bs, fp32):
    """Ties under the MFMA setup's pivot rule (the scalar kernel's), at test_mfma_setup_pivoting's
    tolerance."""
    csr = cases.pivot_blocks(bs, 0, True, fp32)
    A, n = _op(vk_lib, gpu, csr)
    M = vk_lib.block_jacobi(A, bs, setup="mfma")
    _blocks_close(M.inverse(), coracle.bj_setup(*csr, bs), bs, 1e-11)
    _blocks_close(M.inverse(), twin.bj_inverse_numpy(*csr, n, bs), bs, 1e-11)
    M.close()
    A.close()


@pytest.mark.parametrize("block", [2, -1], ids=["inner", "padded"])
@pytest.mark.parametrize("kind", ["col", "row"])
@pytest.mark.parametrize("bs", [7, 8, 33, 64])
def test_singular_block_raises(gpu, vk_lib, bs, kind, block):
    """An exact zero pivot (bs 8: the lane kernel; 7, 33, 64: the generic kernel) is reported, with
    the oracle's block number."""
    csr = cases.singular_blocks(bs, kind, block)
    A, n = _op(vk_lib, gpu, csr)
    nb = (n + bs - 1) // bs
    with pytest.raises(np.linalg.LinAlgError, match=f"singular diagonal block {block % nb}$"):
        coracle.bj_setup(*csr, bs)
    with pytest.raises(np.linalg.LinAlgError, match=f"singular diagonal block {block % nb}$"):
        vk_lib.block_jacobi(A, bs, setup="exact")
    A.close()


def _solver_bars(vk, A, M, csr, inv, n):
    b = twin.rhs(n)
    ref = coracle.gmres(*csr, b, inv, rtol=1e-10)
    xd = np.linalg.solve(cases.dense(*csr), b)
    assert ref.info == 0 and np.linalg.norm(ref.x - xd) / np.linalg.norm(xd) <= 1e-9
    for orth in ("mgs", "dcgs2"):
        x, info = vk.gmres(A, b, rtol=1e-10, M=M, orth=orth)
        st = vk.last_stats()
        assert info == ref.info
        assert abs(st.inner_iters - ref.inner_iters) <= 1, (orth, st.inner_iters, ref.inner_iters)
        rel = np.linalg.norm(x - ref.x) / np.linalg.norm(ref.x)
        assert rel <= 1e-9, (orth, rel)


@pytest.mark.parametrize("bs", [2, 4, 8])
def test_tri_check_accepts_accurate_factors(gpu, vk_lib, bs):
    """d0 = 1e-4: Thomas without pivoting is > 50x inside the check's bound
    (test_oracle_cases.test_tri_blocks_margins): the tridiagonal apply stays available.  Its
    factors carry ~1e-12 of error here (growth 1 / d0), the size of the apply bar itself; the
    builder's seeds are those at which the host restatement of the apply keeps half the bar
    (cases.TRI_SEED).  Measured at other seeds: 0.7 .. 1.5 x the bar, on the device as on the host."""
    csr = cases.tri_blocks(bs, 1e-4)
    A, n = _op(vk_lib, gpu, csr)
    M = vk_lib.block_jacobi(A, bs)
    assert M.tridiag_available and M.mode == "tridiag"
    inv = coracle.bj_setup(*csr, bs)
    assert np.array_equal(M.inverse(), inv)
    b = twin.rhs(n)
    ref = coracle.bj_apply(inv, b)
    np.testing.assert_allclose(M @ b, ref, rtol=1e-12, atol=1e-14 * np.abs(ref).max())
    _solver_bars(vk_lib, A, M, csr, inv, n)
    M.close()
    A.close()


@pytest.mark.parametrize("bs,d0", [(2, 1e-8), (4, 1e-8), (8, 1e-8), (2, 0.0)])
def test_tri_check_rejects_inaccurate_factors(gpu, vk_lib, bs, d0):
    """Tridiagonal, well-conditioned blocks on which Thomas without pivoting is > 50x outside the
    check's bound (d0 = 1e-8) or divides by a zero leading pivot (d0 = 0): the fast apply must not
    be used."""
    csr = cases.tri_blocks(bs, d0)
    A, n = _op(vk_lib, gpu, csr)
    M = vk_lib.block_jacobi(A, bs)
    assert not M.tridiag_available
    assert M.mode == "inverse"
    with pytest.raises(ValueError):
        M.set_mode("tridiag")
    assert M.mode == "inverse"
    inv = coracle.bj_setup(*csr, bs)
    assert np.array_equal(M.inverse(), inv)
    b = twin.rhs(n)
    assert np.array_equal(M @ b, coracle.bj_apply(inv, b))
    _solver_bars(vk_lib, A, M, csr, inv, n)
    M.close()
    A.close()


# ---- w = M^-1 (A x): vtk_precond_matvec ---------------------------------------------------


def _pin(vk, A, csr, n, bs):
    """precond_matvec == the oracle's bj_apply(inv, spmv(x)) == M @ (A @ x), bit for bit, in every
    layout (inverse mode)."""
    x = twin.rhs(n, seed=0xC0FFEE)
    y = coracle.spmv(*csr, x)
    inv = coracle.bj_setup(*csr, bs)
    want = coracle.bj_apply(inv, y)
    for layout in LAYOUTS:
        A.set_layout(layout)
        assert A.layout == layout
        M = vk.block_jacobi(A, bs, mode="inverse", setup="exact")
        assert np.array_equal(A @ x, y), layout
        assert np.array_equal(A.precond_matvec(None, x), y), layout
        w = A.precond_matvec(M, x)
        assert np.array_equal(w, want), (layout, np.abs(w - want).max())
        assert np.array_equal(M @ (A @ x), want), layout
        M.close()


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("bs", FUSED_BS + SPLIT_BS)
def test_precond_matvec_pivot_blocks(gpu, vk_lib, bs, fp32):
    csr = cases.pivot_blocks(bs, 0, False, fp32)
    A, n = _op(vk_lib, gpu, csr)
    _pin(vk_lib, A, csr, n, bs)
    A.close()


@pytest.mark.parametrize("bs", FUSED_BS + SPLIT_BS)
def test_precond_matvec_ragged(gpu, vk_lib, golden, bs):
    """General CSR: ragged rows (empty ones, a 2500-entry one), n = 3000 (a padded last block for
    every bs but 1, 2, 3, 4, 8)."""
    csr = (golden["ragged/indptr"], golden["ragged/indices"], golden["ragged/data"])
    A, n = _op(vk_lib, gpu, csr)
    _pin(vk_lib, A, csr, n, bs)
    A.close()


@pytest.mark.parametrize("bs", [2, 4, 8])
@pytest.mark.parametrize("name", ["S2", "C0"])
def test_precond_matvec_tridiag_mode(gpu, vk_lib, name, bs):
    """Tridiagonal mode.  CSR layout: the epilogue solves with the stored factors l | m | g as the
    stand-alone apply does -- bit-identical to M @ (A @ x).  SELL layouts: the epilogue reads m
    alone and forms l_i = sub_i * m_{i-1} from the row's own entry (bj_trim_group), where the
    stored factor is sub_i / u_{i-1}: the same solve to rounding, not bit for bit (measured:
    max |w - M(Ax)| = 2.2e-16 on S2, 5.6e-16 on C0 bs 8, at max|w| ~ 1.8; equal on C0 bs 2 / 4),
    so there it is held to the tridiagonal apply's bar against the oracle (test_bj_tridiag_apply:
    1e-12 relative, 1e-14 max|w| absolute), as is every layout's split form."""
    p = twin.CONFIGS[name]
    A = vk_lib.vlasov_operator(vk_lib.vlasov_params(p.dim, p.shape), ctx=gpu)
    csr = A.download()
    x = twin.rhs(p.n, seed=0xC0FFEE)
    y = coracle.spmv(*csr, x)
    want = coracle.bj_apply(coracle.bj_setup(*csr, bs), y)
    for layout in LAYOUTS:
        A.set_layout(layout)
        M = vk_lib.block_jacobi(A, bs, mode="tridiag")
        assert M.mode == "tridiag"
        w = A.precond_matvec(M, x)
        split = M @ (A @ x)
        print(f"\n{name} bs {bs} {layout}: max |fused - split| = {np.abs(w - split).max():.3e}, "
              f"max |fused - oracle| = {np.abs(w - want).max():.3e}, max |w| = {np.abs(want).max():.3e}")
        np.testing.assert_allclose(split, want, rtol=1e-12, atol=1e-14 * np.abs(want).max())
        np.testing.assert_allclose(w, want, rtol=1e-12, atol=1e-14 * np.abs(want).max())
        if layout == "csr":
            assert np.array_equal(w, split), layout
        M.close()
    A.close()
