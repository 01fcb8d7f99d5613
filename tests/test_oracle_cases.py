"""The CPU oracle on the inputs of oracle/cases.py (no GPU): blocks that need a row swap in every
column, exactly singular blocks, tridiagonal blocks at both sides of the setup's factor check,
and operators whose GMRES convergence depends on the high Arnoldi columns.  The GPU tests
(test_gpu_bj_pivot.py, test_gpu_arnoldi_edges.py) compare the device with the oracle on these
inputs; here the oracle itself is compared with numpy.linalg.inv and SciPy's gmres on them."""
import numpy as np
import pytest

from oracle import cases, coracle, twin

PIVOT_BS = [1, 2, 3, 4, 5, 7, 8, 12, 16, 32, 33, 63, 64]


def _blocks_close(got, ref, bs, tol):
    """test_gpu_bj_mfma._blocks_close: error relative to each block's largest inverse entry."""
    g = got.reshape(-1, bs, bs)
    r = ref.reshape(-1, bs, bs)
    scale = np.abs(r).max(axis=(1, 2), keepdims=True)
    err = np.abs(g - r) / scale
    assert err.max() <= tol, err.max()


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("ints", [False, True], ids=["normal", "ints"])
@pytest.mark.parametrize("bs", PIVOT_BS)
def test_pivot_blocks_shape(bs, ints, fp32):
    """The builder delivers what the GPU tests rely on: zero block diagonals (a swap in every
    column), a padded last block, the off-block entries, one non-canonical row."""
    ip, ix, d = cases.pivot_blocks(bs, 0, ints, fp32)
    n = ip.shape[0] - 1
    assert n == cases.pivot_n(bs) and (bs == 1 or n % bs != 0)
    assert d.dtype == (np.float32 if fp32 else np.float64)
    A = cases.dense(ip, ix, d)
    assert A[0, n - 1] == 3.0 and A[n - 1, 0] == -2.0
    B = twin.bj_blocks(ip, ix, d, n, bs)
    for k in range(B.shape[0]):
        m = min(bs, n - k * bs)
        if m > 1:
            assert np.all(np.diag(B[k])[:m] == 0.0)
        assert np.linalg.matrix_rank(B[k]) == bs and np.linalg.cond(B[k][:m, :m]) < 1e4
    r = 1 if bs == 1 else bs + 1
    row = ix[ip[r]:ip[r + 1]]
    assert np.any(np.diff(row) < 0) and len(set(row.tolist())) < row.shape[0]
    if ints:
        assert np.all(B == np.round(B)) and np.abs(B).max() <= 4   # many exact |a| ties


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("ints", [False, True], ids=["normal", "ints"])
@pytest.mark.parametrize("bs", PIVOT_BS)
def test_c_bj_setup_pivoting_vs_numpy(bs, ints, fp32):
    """orc_bj_setup (Gauss-Jordan, first row of largest |a|) against LAPACK's inverse where every
    column swaps rows: test_gpu_bj_mfma's measure at its pivoting tolerance (measured worst over
    all cases: 1.7e-13)."""
    ip, ix, d = cases.pivot_blocks(bs, 0, ints, fp32)
    n = ip.shape[0] - 1
    inv = coracle.bj_setup(ip, ix, d, bs)
    _blocks_close(inv, twin.bj_inverse_numpy(ip, ix, d, n, bs), bs, 1e-11)
    # and it is an inverse: B inv = I to the blocks' conditioning (cond < 1e4)
    B = twin.bj_blocks(ip, ix, d, n, bs)
    res = np.abs(np.einsum("bij,bjk->bik", B, inv) - np.eye(bs)).max()
    assert res <= 1e-10, res


@pytest.mark.parametrize("block", [2, -1], ids=["inner", "padded"])
@pytest.mark.parametrize("kind", ["col", "row"])
@pytest.mark.parametrize("bs", [7, 8, 33, 64])
def test_c_bj_setup_singular(bs, kind, block):
    ip, ix, d = cases.singular_blocks(bs, kind, block)
    n = ip.shape[0] - 1
    nb = (n + bs - 1) // bs
    B = twin.bj_blocks(ip, ix, d, n, bs)
    assert np.linalg.matrix_rank(B[block % nb]) == bs - 1
    with pytest.raises(np.linalg.LinAlgError, match=f"singular diagonal block {block % nb}$"):
        coracle.bj_setup(ip, ix, d, bs)


def _thomas(bs, d0):
    ip, ix, d = cases.tri_blocks(bs, d0)
    n = ip.shape[0] - 1
    B = twin.bj_blocks(ip, ix, d, n, bs)
    # the blocks are tridiagonal (reason 1 of the setup's check does not apply)
    i, j = np.indices((bs, bs))
    assert not B[:, np.abs(i - j) > 1].any()
    inv = coracle.bj_setup(ip, ix, d, bs)
    _blocks_close(inv, np.linalg.inv(B), bs, 1e-12)
    return B, [cases.thomas_check(B[k], inv[k]) for k in range(B.shape[0])]


@pytest.mark.parametrize("bs", [2, 4, 8])
def test_tri_blocks_margins(bs):
    """The device setup accepts the tridiagonal apply when Thomas without pivoting reproduces the
    Gauss-Jordan inverse within 1e-10 of its largest entry.  Restated here (cases.thomas_check):
    the d0 = 1e-8 input is more than 50x over that bound, the d0 = 1e-4 input more than 50x under
    it, and neither trips the tiny-pivot reason, so what the GPU test expects is not borderline."""
    B, chk = _thomas(bs, 1e-8)
    assert max(np.linalg.cond(b) for b in B) <= 40          # Thomas is inaccurate, the block is fine
    assert not any(t for t, _, _ in chk)
    worst = max(e / m for _, e, m in chk)
    assert worst >= 50 * 1e-10, worst
    B, chk = _thomas(bs, 1e-4)
    assert max(np.linalg.cond(b) for b in B) <= 40
    assert not any(t for t, _, _ in chk)
    worst = max(e / m for _, e, m in chk)
    assert worst <= 1e-10 / 50, worst
    # the accepted factors applied (the device's scan order restated) stay within half of the
    # suite's tridiagonal-apply bar of the inverse apply: the GPU test holds the device to the
    # whole bar (cases.TRI_SEED: the seeds were chosen for this)
    ip, ix, d = cases.tri_blocks(bs, 1e-4)
    b = twin.rhs(ip.shape[0] - 1)
    ref = coracle.bj_apply(coracle.bj_setup(ip, ix, d, bs), b)
    z = np.concatenate([cases.tri_scan_apply(*cases.thomas_factors(B[k])[:3], b[k * bs:(k + 1) * bs])
                        for k in range(B.shape[0])])
    np.testing.assert_allclose(z, ref, rtol=0.5e-12, atol=0.5e-14 * np.abs(ref).max())


def test_tri_blocks_zero_leading_pivot():
    """d0 = 0, bs 2: nonsingular blocks (cond < 10) whose leading Thomas pivot is exactly zero."""
    B, chk = _thomas(2, 0.0)
    assert max(np.linalg.cond(b) for b in B) < 10
    assert all(t for t, _, _ in chk)


# ---- GMRES -------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def R():
    ip, ix, d = cases.op_R()
    n = ip.shape[0] - 1
    b = twin.rhs(n)
    return ip, ix, d, b, np.linalg.solve(cases.dense(ip, ix, d), b)


# restart: (info, inner iterations) of the C oracle on R at rtol 1e-10, maxiter 40
R_COUNTS = {20: (40, 800), 31: (0, 243), 32: (0, 253), 40: (0, 123)}


@pytest.mark.parametrize("restart", [31, 32, 40])
def test_c_gmres_R_vs_scipy(R, restart):
    """On R the iteration count depends on the high columns of every cycle (restart 20 does not
    converge in 800 iterations, 32 takes 253, 40 takes 123): the oracle against SciPy's gmres."""
    ip, ix, d, b, xd = R
    n = b.shape[0]
    ref = coracle.gmres(ip, ix, d, b, None, rtol=1e-10, restart=restart, maxiter=40)
    assert (ref.info, ref.inner_iters) == R_COUNTS[restart]
    s = twin.scipy_gmres(twin.scipy_csr(ip, ix, d, n), b, None, rtol=1e-10, restart=restart, maxiter=40)
    assert s.info == ref.info
    assert abs(s.inner_iters - ref.inner_iters) <= 1, (s.inner_iters, ref.inner_iters)
    assert np.linalg.norm(s.x - ref.x) / np.linalg.norm(ref.x) <= 1e-9
    # converged to the dense solution as far as cond ~ 4.8e3 and rtol 1e-10 allow
    assert np.linalg.norm(ref.x - xd) / np.linalg.norm(xd) <= 5e-9


def test_c_gmres_R_restart20_stalls(R):
    ip, ix, d, b, xd = R
    ref = coracle.gmres(ip, ix, d, b, None, rtol=1e-10, restart=20, maxiter=40)
    assert (ref.info, ref.inner_iters) == R_COUNTS[20]
    assert np.linalg.norm(ref.x - xd) / np.linalg.norm(xd) > 1e-2


def test_c_gmres_Q_converges():
    """Q (cond ~ 1e6): counts depend on the Gram-Schmidt variant (oracle 87, SciPy 92 at restart
    32), so only convergence is pinned."""
    ip, ix, d = cases.op_Q()
    n = ip.shape[0] - 1
    b = twin.rhs(n)
    ref = coracle.gmres(ip, ix, d, b, None, rtol=1e-10, restart=32, maxiter=40)
    assert ref.info == 0 and ref.restarts <= 4
    assert np.linalg.norm(b - coracle.spmv(ip, ix, d, ref.x)) <= 1e-10 * np.linalg.norm(b) * 1.0001


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_c_gmres_low_degree(k):
    """k distinct eigenvalues: exactly k iterations, to rounding."""
    ip, ix, d = cases.low_degree_diag(k)
    b = twin.rhs(ip.shape[0] - 1)
    ref = coracle.gmres(ip, ix, d, b, None, rtol=1e-12, restart=20)
    assert ref.info == 0 and ref.inner_iters == k
    assert np.linalg.norm(ref.x - b / d) / np.linalg.norm(b / d) <= 1e-14
