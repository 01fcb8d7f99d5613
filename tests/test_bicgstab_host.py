"""BiCGStab without a GPU: the NumPy twin of scipy.sparse.linalg.bicgstab that the GPU tests use as
their reference (pinned to SciPy bit for bit here), the argument validation of ``vtkrylov.bicgstab``
(all of it happens before anything touches a device), the C entry's NULL check, and the entry
layer's ``solver/method`` switch.
"""
import functools
import os

import numpy as np
import pytest

from oracle import coracle, twin


def bicgstab_twin(A, b, x0=None, *, rtol=1e-5, atol=0.0, maxiter=None, M=None, dot=np.dot):
    """scipy.sparse.linalg.bicgstab restated (iterative.py, SciPy 1.15): returns (x, info,
    iterations, half_step) with iterations = v = A M p products that count (a top exit or a
    breakdown at loop index k: k; the half-step exit: k + 1) -- SciPy's callback count is
    iterations - half_step.  M: None or a callable r -> M r."""
    b = np.asarray(b, dtype=np.float64)
    n = b.shape[0]
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    psolve = (lambda y: y) if M is None else M
    norm = lambda y: np.sqrt(dot(y, y))
    bnrm2 = norm(b)
    atol = max(float(atol), float(rtol) * float(bnrm2))
    if bnrm2 == 0:
        return b.copy(), 0, 0, 0
    maxiter = n * 10 if maxiter is None else maxiter
    tol2 = np.finfo(np.float64).eps ** 2
    r = b - A @ x if x.any() else b.copy()
    rtilde = r.copy()
    rho_prev = omega = alpha = p = v = None
    for k in range(maxiter):
        if norm(r) < atol:
            return x, 0, k, 0
        rho = dot(rtilde, r)
        if np.abs(rho) < tol2:
            return x, -10, k, 0
        if k > 0:
            if np.abs(omega) < tol2:
                return x, -11, k, 0
            beta = (rho / rho_prev) * (alpha / omega)
            p -= omega * v
            p *= beta
            p += r
        else:
            p = r.copy()
        phat = psolve(p)
        v = A @ phat
        rv = dot(rtilde, v)
        if rv == 0:
            return x, -11, k, 0
        alpha = rho / rv
        r -= alpha * v          # s, in place
        if norm(r) < atol:
            x += alpha * phat
            return x, 0, k + 1, 1
        shat = psolve(r)
        t = A @ shat
        omega = dot(t, r) / dot(t, t)
        x += alpha * phat
        x += omega * shat
        r -= omega * t
        rho_prev = rho
    return x, maxiter, maxiter, 0


LINE = {"S2": (32, 25), "S4": (320, 3), "C0": (1, 25)}   # line stride, segment


@functools.lru_cache(maxsize=None)
def host_case(name):
    p = twin.CONFIGS[name]
    ip, ix, d = coracle.generate(p)
    return p, ip, ix, d, twin.scipy_csr(ip, ix, d.astype(np.float64), p.n), twin.rhs(p.n)


def host_prec(name, kind):
    p, ip, ix, d, A, b = host_case(name)
    if kind == "none":
        return None
    if kind == "bj":
        return twin.bj_operator(twin.bj_inverse_numpy(ip, ix, d, p.n, 8), p.n)
    return twin.line_operator(ip, ix, d, p.n, *LINE[name])


@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
@pytest.mark.parametrize("kind", ["none", "bj", "line"])
@pytest.mark.parametrize("name", ["S2", "S4", "C0"])
def test_twin_is_scipy_bit_for_bit(name, kind, rtol):
    from scipy.sparse.linalg import bicgstab
    p, ip, ix, d, A, b = host_case(name)
    M = host_prec(name, kind)
    calls = [0]

    def cb(_):
        calls[0] += 1

    xs, infos = bicgstab(A, b, rtol=rtol, atol=0.0, M=M, callback=cb, maxiter=2000)
    x, info, its, half = bicgstab_twin(A, b, rtol=rtol, M=None if M is None else M.matvec, maxiter=2000)
    assert info == infos == 0
    assert np.array_equal(x, xs), np.linalg.norm(x - xs) / np.linalg.norm(xs)
    assert its - half == calls[0], (its, half, calls[0])


def test_twin_exits_of_the_line_cases():
    """The two exits the GPU tests pin: S2 / line at rtol 1e-8 leaves through the half step."""
    p, ip, ix, d, A, b = host_case("S2")
    x, info, its, half = bicgstab_twin(A, b, rtol=1e-8, M=host_prec("S2", "line").matvec)
    assert (info, its, half) == (0, 8, 1)


def test_twin_truncated_zero_b_and_breakdowns():
    from scipy.sparse.linalg import bicgstab
    p, ip, ix, d, A, b = host_case("S2")
    xs, infos = bicgstab(A, b, rtol=1e-8, maxiter=3)
    x, info, its, half = bicgstab_twin(A, b, rtol=1e-8, maxiter=3)
    assert info == infos == 3 and its == 3 and np.array_equal(x, xs)
    x, info, its, half = bicgstab_twin(A, np.zeros(p.n), x0=b)
    assert not x.any() and (info, its) == (0, 0)
    for A3, b3, want in BREAKDOWNS:
        A3 = np.array(A3, dtype=np.float64)
        b3 = np.array(b3, dtype=np.float64)
        xs, infos = bicgstab(A3, b3, rtol=1e-12)
        x, info, its, half = bicgstab_twin(A3, b3, rtol=1e-12)
        assert (info, its) == want and infos == info and np.array_equal(x, xs)


# exact breakdowns (every intermediate dyadic): matrix, right-hand side, (info, iterations)
BREAKDOWNS = [
    ([[-1, -1, -1], [0, 2, -1], [-1, -1, 0]], [1, 1, 0], (-11, 0)),    # <rtilde, v> == 0
    ([[-1, -1, -1], [-1, -1, 0], [2, 0, 0]], [1, 0, 0], (-11, 1)),     # omega == 0
    ([[-1, -1, -1], [-1, -1, 0], [-1, 0, 0]], [1, 1, 0], (-10, 1)),    # rho == 0
]


# ---- the general CSR case of the GPU tests -------------------------------------------------

@functools.lru_cache(maxsize=None)
def general_csr():
    """Random non-symmetric, strictly diagonally dominant: n = 1000, 1-12 entries per row, the
    diagonal positive (sum of the row's |off-diagonals| + 1).  The sign matters: with diagonals of
    random sign the matrix is indefinite, BiCGStab converges erratically, and the twin's own count
    moves with the summation order of its dots alone (138 / 150 / 168 iterations at rtol 1e-5 for
    the three orders below) -- no fixed-order device sum can be held to a 15 % bar there."""
    import scipy.sparse as sp
    rng = np.random.default_rng(20240607)
    n = 1000
    rows, cols, vals = [], [], []
    for i in range(n):
        k = int(rng.integers(0, 12))                      # off-diagonal entries; + the diagonal
        c = rng.choice(np.delete(np.arange(n), i), size=k, replace=False)
        v = rng.standard_normal(k)
        rows += [i] * (k + 1)
        cols += list(c) + [i]
        vals += list(v) + [np.abs(v).sum() + 1.0]
    R = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    R.sort_indices()
    return R


def dot_strided(a, c):
    """509 strided partials summed in reverse."""
    pr = a * c
    s = 0.0
    for v in reversed([pr[i::509].sum() for i in range(509)]):
        s += v
    return s


def dot_running(a, c):
    s = 0.0
    for v in (a * c).tolist():
        s += v
    return s


@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
def test_general_csr_case_is_stable_under_summation_order(rtol):
    """The premise of the GPU test's bars on this matrix, checked on the reference itself: the
    twin's count and iterate under three summation orders of its dots stay inside them."""
    R = general_csr()
    per_row = np.diff(R.indptr)
    assert per_row.min() >= 1 and per_row.max() <= 12 and (R != R.T).nnz > 0
    off = abs(R).sum(axis=1).A1 - abs(R.diagonal())
    assert (R.diagonal() > off).all()
    b = twin.rhs(R.shape[0])
    runs = [bicgstab_twin(R, b, rtol=rtol, maxiter=500, dot=d) for d in (np.dot, dot_strided, dot_running)]
    x0, info0, its0, _ = runs[0]
    for x, info, its, _ in runs[1:]:
        assert info == info0 == 0
        assert abs(its - its0) <= max(2, int(np.ceil(0.15 * its0)))
        assert np.linalg.norm(x - x0) <= 4 * rtol * np.linalg.norm(x0)


# ---- vtkrylov.bicgstab: arguments, before any device work ------------------------------------

def test_name_is_public(vk_lib):
    for name in ("bicgstab", "BicgstabStats", "last_bicgstab_stats"):
        assert name in vk_lib.__all__ and hasattr(vk_lib, name)
    assert vk_lib.last_bicgstab_stats() is None or isinstance(vk_lib.last_bicgstab_stats(), vk_lib.BicgstabStats)


def test_argument_validation_needs_no_gpu(vk_lib):
    import scipy.sparse as sp
    from scipy.sparse.linalg import LinearOperator
    A = sp.identity(4, format="csr")
    b = np.ones(4)
    with pytest.raises(NotImplementedError):
        vk_lib.bicgstab(A, b, callback=lambda x: None)
    with pytest.raises(TypeError):
        vk_lib.bicgstab(A, b, M=LinearOperator((4, 4), matvec=lambda r: r))
    for atol in (-1, None, "legacy"):
        with pytest.raises(ValueError, match="'scipy.sparse.linalg.bicgstab' called with invalid `atol`"):
            vk_lib.bicgstab(A, b, atol=atol)
    for maxiter in (0, 2.5):
        with pytest.raises(ValueError, match="maxiter"):
            vk_lib.bicgstab(A, b, maxiter=maxiter)


def test_c_entry_rejects_null(vk_lib):
    L = vk_lib._abi.lib()
    assert L.vtk_bicgstab(None, None, None, None, 1e-5, 0.0, 0, 0, None, None) == vk_lib._abi.ERR_ARG


# ---- entry layer ---------------------------------------------------------------------------

def test_solver_method_switch(tmp_path):
    from vtsetup.config import DEFAULT_XML, SolverConfig
    assert SolverConfig.load().method == "gmres"
    assert SolverConfig.load(method="bicgstab").method == "bicgstab"
    with pytest.raises(ValueError):
        SolverConfig.load(method="cg")
    with pytest.raises(ValueError, match="one rank"):
        SolverConfig.load(method="bicgstab", gpus=2)
    # a configuration written before the node existed
    lines = [ln for ln in open(DEFAULT_XML) if "<method>" not in ln]
    assert len(lines) == len(open(DEFAULT_XML).readlines()) - 1
    old = tmp_path / "old.xml"
    old.write_text("".join(lines))
    assert SolverConfig.load(str(old)).method == "gmres"
    assert SolverConfig.load(str(old), method="bicgstab").method == "bicgstab"


def test_entry_refuses_bicgstab_across_ranks(capsys):
    from vtsetup.krylov_precondition import test_main as entry
    assert entry(["--config", "S2", "--method", "bicgstab", "--gpus", "2", "--dry-run"]) == 2
    assert "one rank" in capsys.readouterr().err
