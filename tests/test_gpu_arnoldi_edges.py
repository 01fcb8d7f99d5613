"""The Arnoldi process at its edges, both orthogonalisations against the C oracle (SciPy's MGS
sequence) and dense host solves:

* every restart length at which the DCGS2 kernels change form (k_dc_dots_rows<8 | 16 | 24 | 32>:
  j = 8 | 9, 16 | 17, 24 | 25; the DCGS2 limit 32 | 33) and the restarts that divide the
  iteration count, so that convergence lands on a cycle's last column;
* R (oracle/cases.py): an operator whose iteration count depends on the columns past 24 of
  every cycle -- restart 20 does not converge at all, 31 / 32 / 40 take 243 / 253 / 123;
* Q: the same at cond ~ 1e6 (weak bars);
* operators with k distinct eigenvalues: the Krylov space is exhausted at step k (the breakdown
  branch of the scalar step, its r2 <= 0 and nu fallbacks);
* x0 already the solution.
"""
import numpy as np
import pytest

from oracle import cases, coracle, twin

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["mgs", "dcgs2"])
def orth(request, gpu, vk_lib):
    """test_gpu_parity's pattern: the context's scheme is forced for the test."""
    gpu.set_orth({"mgs": vk_lib._abi.ORTH_MGS, "dcgs2": vk_lib._abi.ORTH_DCGS2}[request.param])
    yield request.param
    gpu.set_orth(vk_lib._abi.ORTH_AUTO)


def _check_solve(xg, info, st, ref, tol=1e-9):
    assert info == ref.info, (info, ref.info)
    assert abs(st.inner_iters - ref.inner_iters) <= 1, (st.inner_iters, ref.inner_iters)
    rel = np.linalg.norm(xg - ref.x) / np.linalg.norm(ref.x)
    assert rel <= tol, rel


# ---- restart sweep on S2 -------------------------------------------------------------------


@pytest.fixture(scope="module")
def s2(gpu, vk_lib):
    p = twin.CONFIGS["S2"]
    A = vk_lib.vlasov_operator(vk_lib.vlasov_params(p.dim, p.shape), ctx=gpu)
    csr = A.download()
    M = vk_lib.block_jacobi(A, 8)
    inv = coracle.bj_setup(*csr, 8)
    assert np.array_equal(M.inverse(), inv)
    refs = {}

    def ref(prec, restart):
        if (prec, restart) not in refs:      # one oracle solve per case, shared by both orths
            refs[prec, restart] = coracle.gmres(*csr, twin.rhs(p.n), inv if prec else None, rtol=1e-8,
                                                restart=restart)
        return refs[prec, restart]

    yield A, M, csr, twin.rhs(p.n), ref
    M.close()
    A.close()


SWEEP = [1, 2, 4, 8, 9, 16, 17, 24, 25, 31, 32]


@pytest.mark.parametrize("prec", [True, False], ids=["bj8", "noprec"])
@pytest.mark.parametrize("restart", SWEEP)
def test_restart_sweep(vk_lib, s2, orth, restart, prec):
    """With BJ(8) the oracle takes 68 iterations at every restart from 4 on: restarts 4 and 17
    divide it (convergence on the last column of a cycle: the scalar step's `last` commit)."""
    A, M, csr, b, ref = s2
    r = ref(prec, restart)
    assert r.info == 0
    if prec and restart >= 4:
        assert r.inner_iters == 68
    x, info = vk_lib.gmres(A, b, rtol=1e-8, restart=restart, M=M if prec else None)
    st = vk_lib.last_stats()
    assert st.orth == (0 if orth == "mgs" else 1)
    _check_solve(x, info, st, r)
    assert st.breakdown == 0
    assert np.linalg.norm(b - coracle.spmv(*csr, x)) <= 1e-8 * np.linalg.norm(b) * 1.0001


@pytest.mark.parametrize("prec", [True, False], ids=["bj8", "noprec"])
@pytest.mark.parametrize("restart", [32, 33, 34])
def test_restart_past_dcgs2_limit(vk_lib, s2, restart, prec):
    """Auto: DCGS2 up to restart 32, MGS beyond (34 divides the 68 iterations); forcing DCGS2
    beyond its limit is an error, not a silent switch."""
    A, M, csr, b, ref = s2
    r = ref(prec, restart)
    x, info = vk_lib.gmres(A, b, rtol=1e-8, restart=restart, M=M if prec else None)
    st = vk_lib.last_stats()
    assert st.orth == (1 if restart <= 32 else 0)
    _check_solve(x, info, st, r)
    if restart > 32:
        x2, info2 = vk_lib.gmres(A, b, rtol=1e-8, restart=restart, M=M if prec else None, orth="mgs")
        _check_solve(x2, info2, vk_lib.last_stats(), r)
        with pytest.raises(ValueError):
            vk_lib.gmres(A, b, rtol=1e-8, restart=restart, M=M if prec else None, orth="dcgs2")


def test_x0_already_the_solution(vk_lib, s2, orth):
    """iterative.py:741: ||b - A x0|| < atol returns x0 untouched, no Arnoldi step."""
    A, M, csr, b, ref = s2
    x, info = vk_lib.gmres(A, b, rtol=1e-8, M=M)
    assert info == 0
    r = coracle.gmres(*csr, b, coracle.bj_setup(*csr, 8), rtol=1e-8, x0=x)
    assert (r.info, r.inner_iters) == (0, 0) and np.array_equal(r.x, x)
    x2, info2 = vk_lib.gmres(A, b, x0=x, rtol=1e-8, M=M)
    st = vk_lib.last_stats()
    assert info2 == 0 and st.inner_iters == 0
    assert np.array_equal(x2, x)


# ---- R and Q: the high columns decide ----------------------------------------------------------


class _Outlier:
    def __init__(self, vk, gpu, csr):
        self.csr = csr
        self.n = csr[0].shape[0] - 1
        self.A = vk.csr_matrix((csr[2], csr[1], csr[0]), shape=(self.n, self.n), ctx=gpu)
        self.b = twin.rhs(self.n)
        self.xd = np.linalg.solve(cases.dense(*csr), self.b)
        self.refs = {}

    def ref(self, restart, maxiter=40):
        k = (restart, maxiter)
        if k not in self.refs:
            self.refs[k] = coracle.gmres(*self.csr, self.b, None, rtol=1e-10, restart=restart, maxiter=maxiter)
        return self.refs[k]

    def err(self, x):
        return np.linalg.norm(x - self.xd) / np.linalg.norm(self.xd)

    def resid(self, x):
        return np.linalg.norm(self.b - coracle.spmv(*self.csr, x))


@pytest.fixture(scope="module")
def opR(gpu, vk_lib):
    o = _Outlier(vk_lib, gpu, cases.op_R())
    yield o
    o.A.close()


@pytest.fixture(scope="module")
def opQ(gpu, vk_lib):
    o = _Outlier(vk_lib, gpu, cases.op_Q())
    yield o
    o.A.close()


def _solve_R(vk, o, restart, orth):
    r = o.ref(restart)
    x, info = vk.gmres(o.A, o.b, rtol=1e-10, restart=restart, maxiter=40)
    st = vk.last_stats()
    print(f"\nR restart {restart} {orth}: info {info} inner {st.inner_iters} restarts {st.restarts} "
          f"(oracle {r.info} / {r.inner_iters} / {r.restarts}); err vs dense {o.err(x):.3e} (oracle {o.err(r.x):.3e}); "
          f"true resid / ||b|| {o.resid(x) / np.linalg.norm(o.b):.3e}")
    return r, x, info, st


@pytest.mark.parametrize("restart", [32, 31])
def test_R_high_columns(vk_lib, opR, orth, restart):
    """GMRES(20) stalls on R (oracle: 800 iterations, error 4e-2) and GMRES(31 / 32) converges in
    243 / 253: a cycle's columns 24 .. 31 (k_dc_dots_rows<32>, k_dc_update and the scalar step at
    j >= 25) carry the convergence, so a defect there moves the count far outside +-1."""
    o = opR
    r, x, info, st = _solve_R(vk_lib, o, restart, orth)
    assert r.info == 0 and r.inner_iters == {31: 243, 32: 253}[restart]
    assert info == r.info
    assert abs(st.inner_iters - r.inner_iters) <= 1, (st.inner_iters, r.inner_iters)
    assert o.err(x) <= 2 * o.err(r.x), (o.err(x), o.err(r.x))
    assert o.resid(x) <= 1e-10 * np.linalg.norm(o.b) * 1.0001
    x2, info2 = vk_lib.gmres(o.A, o.b, rtol=1e-10, restart=restart, maxiter=40)
    assert info2 == info and np.array_equal(x2, x)                # deterministic reductions


def test_R_restart40_mgs(vk_lib, opR):
    o = opR
    r = o.ref(40)
    x, info = vk_lib.gmres(o.A, o.b, rtol=1e-10, restart=40, maxiter=40, orth="mgs")
    st = vk_lib.last_stats()
    assert r.info == 0 and r.inner_iters == 123
    assert info == r.info and st.orth == 0
    assert abs(st.inner_iters - r.inner_iters) <= 1, (st.inner_iters, r.inner_iters)
    assert o.err(x) <= 2 * o.err(r.x), (o.err(x), o.err(r.x))
    assert o.resid(x) <= 1e-10 * np.linalg.norm(o.b) * 1.0001
    x2, _ = vk_lib.gmres(o.A, o.b, rtol=1e-10, restart=40, maxiter=40, orth="mgs")
    assert np.array_equal(x2, x)


def test_R_not_converged(vk_lib, opR, orth):
    """restart 20, maxiter 3: three full cycles without convergence (every cycle ends on its last
    column), x compared at the bar of the info > 0 solves."""
    o = opR
    r = o.ref(20, 3)
    assert (r.info, r.inner_iters) == (3, 60)
    x, info = vk_lib.gmres(o.A, o.b, rtol=1e-10, restart=20, maxiter=3)
    st = vk_lib.last_stats()
    assert info == r.info
    assert st.inner_iters == 60 and st.restarts == 3
    rel = np.linalg.norm(x - r.x) / np.linalg.norm(r.x)
    assert rel <= 1e-8, rel


def test_Q_ill_conditioned(vk_lib, opQ, orth):
    """cond ~ 1e6: the iteration count depends on the Gram-Schmidt variant and its rounding
    (oracle 87, SciPy 92, numpy MGS 84, CGS2 92, CGS 99; measured on the device: MGS 92, DCGS2 92,
    3 cycles each as the oracle), so only convergence is held."""
    o = opQ
    r = o.ref(32)
    assert r.info == 0
    x, info = vk_lib.gmres(o.A, o.b, rtol=1e-10, restart=32, maxiter=40)
    st = vk_lib.last_stats()
    print(f"\nQ restart 32 {orth}: info {info} inner {st.inner_iters} restarts {st.restarts} "
          f"(oracle {r.inner_iters} / {r.restarts}); err vs dense {o.err(x):.3e}")
    assert info == 0
    assert np.all(np.isfinite(x))
    assert o.resid(x) <= 1e-10 * np.linalg.norm(o.b) * 1.0001
    assert st.restarts <= r.restarts + 1, (st.restarts, r.restarts)


# ---- exhausted Krylov space ------------------------------------------------------------------


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_low_degree_converges_in_k(gpu, vk_lib, orth, k):
    """k distinct eigenvalues: the oracle converges in exactly k iterations; the device in k or
    k + 1 (DCGS2 may finalise column k - 1 one step late).  Error bar: cond 14 x rtol 1e-12."""
    csr = cases.low_degree_diag(k)
    n = csr[0].shape[0] - 1
    A = vk_lib.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n), ctx=gpu)
    b = twin.rhs(n)
    xe = b / csr[2]
    r = coracle.gmres(*csr, b, None, rtol=1e-12, restart=20)
    assert r.info == 0 and r.inner_iters == k
    x, info = vk_lib.gmres(A, b, rtol=1e-12, restart=20)
    st = vk_lib.last_stats()
    assert info == 0
    assert np.all(np.isfinite(x))
    assert k <= st.inner_iters <= k + 1, st.inner_iters
    err = np.linalg.norm(x - xe) / np.linalg.norm(xe)
    assert err <= 1e-10, err
    A.close()


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_low_degree_no_tolerance(gpu, vk_lib, orth, k):
    """rtol = atol = 0: nothing stops the Arnoldi process at step k, so it walks into the exhausted
    space -- h_{k+1,k} is zero or rounding noise, the re-orthogonalised norms cancel (the scalar
    step's r2 <= 0 and nu fallbacks).  x must stay finite and exact to the error bar above.

    Measured (inner iterations / restarts, all with breakdown = 1 and info 3):
        k      oracle   device MGS   device DCGS2
        1      1 / 1    1 / 1        1 / 1
        2      37 / 2   2 / 1        2 / 1
        3      42 / 3   42 / 3       29 / 2
        5      44 / 3   45 / 3       43 / 3
    """
    csr = cases.low_degree_diag(k)
    n = csr[0].shape[0] - 1
    A = vk_lib.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n), ctx=gpu)
    b = twin.rhs(n)
    xe = b / csr[2]
    r = coracle.gmres(*csr, b, None, rtol=0.0, atol=0.0, restart=20, maxiter=3)
    x, info = vk_lib.gmres(A, b, rtol=0.0, atol=0.0, restart=20, maxiter=3)
    st = vk_lib.last_stats()
    err = np.linalg.norm(x - xe) / np.linalg.norm(xe)
    print(f"\nlow degree k={k} {orth}: info {info} inner {st.inner_iters} restarts {st.restarts} "
          f"breakdown {st.breakdown} err {err:.3e} (oracle: info {r.info} inner {r.inner_iters} "
          f"restarts {r.restarts})")
    assert np.all(np.isfinite(x))
    assert err <= 1e-10, err
    assert info == r.info == 3            # ||r|| <= 0 is never met: info = maxiter, as the oracle
    assert st.breakdown in (0, 1)
    # The breakdown test is h_{j+1,j} <= eps ||M A v_j|| (iterative.py:766).  Past step k that
    # entry is rounding noise of about that size, so WHEN it trips is noise too: the oracle (SciPy's
    # own sequence) walks 37 .. 44 steps into the exhausted space before it does, over two or three
    # cycles, and the device likewise.  "breakdown => at most k + 1 iterations" therefore holds for
    # no implementation, the reference included; what does hold: a breakdown ends the solve before
    # its 3 x 20 iterations are used up, no breakdown means all of them ran, and never fewer than
    # k steps are taken ...
    if st.breakdown == 1:
        assert k <= st.inner_iters < 60 and st.inner_iters <= 20 * st.restarts, (st.inner_iters, st.restarts)
    else:
        assert st.inner_iters == 60 and st.restarts == 3, (st.inner_iters, st.restarts)
    # ... and for k = 1 (A = I: w = v_0 exactly, h_{1,0} = 0 exactly) the breakdown is exact: it must
    # be flagged at the first column, as the oracle does
    if k == 1:
        assert r.inner_iters == 1
        assert st.breakdown == 1 and st.inner_iters == 1 and st.restarts == 1
    A.close()
