"""Extended-precision reference for the FIRST ITERATIONS of preconditioned BiCGStab -- TEST
INFRASTRUCTURE ONLY (NumPy; nothing in the product imports it).

The solve-level bars (x to 4 rtol, the count to 15 %) cannot see a BiCGStab kernel that is wrong at
the 1e-10 level: the method amplifies summation-order noise over a long run, so the bars are loose.
Its kernels, however, are the same code at every iteration, and over the first three iterations the
method has not amplified anything yet.  This module states those iterations once:

* :class:`Loop`: scipy.sparse.linalg.bicgstab's loop (iterative.py, SciPy 1.15) -- the loop of
  ``tests/test_bicgstab_host.py::bicgstab_twin``, operation for operation, including the three-step
  p update and the two-step x update -- in a chosen precision and with a chosen dot.  Every update
  is a method, so a test can plant a defect in one of them by subclassing.
* :class:`Ops` / :func:`operators`: A and M^-1 in float64 and in ``np.longdouble`` (x87 80-bit) from
  ``oracle.arnoldi.Operator`` (the longdouble M^-1 comes from A's own blocks / line matrix, not
  from any device factors), or M^-1 as a pair of callables (float64, longdouble).
* :func:`figure`: ||x - x_ld|| / ||x_ld||, evaluated in longdouble.
* :func:`reference`: the longdouble run and R_k, the float64 instance's own figure (the worst of
  the given dot orders, floored at the unit roundoff), which sets the bars.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .arnoldi import LD, Operator

U = 2.0 ** -53      # float64 unit roundoff


@dataclass
class Trace:
    """One run.  Entry j of every list belongs to loop index j (iteration j + 1): xs[j], rs[j] the
    iterate and the recurrence residual after it (a half-step exit: the returned x and s), snorm[j]
    = ||s||, and the iteration's alpha, omega (None at a half-step exit) and rho."""
    x: np.ndarray
    info: int
    iterations: int
    half_step: int
    xs: list = field(default_factory=list)
    rs: list = field(default_factory=list)
    snorm: list = field(default_factory=list)
    alpha: list = field(default_factory=list)
    omega: list = field(default_factory=list)
    rho: list = field(default_factory=list)
    rnorm0: object = None          # ||r_0||


class Loop:
    """bicgstab in ``dtype``; A, Minv: callables on ``dtype`` vectors; dot: the sum of the products."""

    def __init__(self, A, Minv, dtype=LD, dot=np.dot):
        self.A, self.Minv, self.dtype, self.dot = A, Minv, dtype, dot

    # -- the steps (SciPy's statements) ------------------------------------------------------
    def norm(self, y):
        return np.sqrt(self.dot(y, y))

    def residual0(self, b, x):
        return b - self.A(x) if x.any() else b.copy()

    def rho(self, k, rtilde, r):
        return self.dot(rtilde, r)

    def beta(self, rho, rho_prev, alpha, omega):
        return (rho / rho_prev) * (alpha / omega)

    def update_p(self, p, r, v, beta, omega):
        p -= omega * v
        p *= beta
        p += r

    def psolve(self, k, which, y):
        """which: "p" (phat = M^-1 p) or "s" (shat = M^-1 s) of loop index k."""
        return self.Minv(y)

    def omega(self, t, s):
        return self.dot(t, s) / self.dot(t, t)

    def update_x(self, x, alpha, phat, omega, shat):
        x += alpha * phat
        x += omega * shat

    def half_x(self, x, alphas, phat):
        x += alphas[-1] * phat

    # -- the loop ----------------------------------------------------------------------------
    def solve(self, b, x0=None, *, rtol=0.0, atol=0.0, maxiter) -> Trace:
        dt = self.dtype
        b = np.asarray(b).astype(dt)
        n = b.shape[0]
        x = np.zeros(n, dt) if x0 is None else np.array(x0).astype(dt)
        bnrm2 = self.norm(b)
        atol = max(dt(atol), dt(rtol) * bnrm2)
        if bnrm2 == 0:
            return Trace(b.copy(), 0, 0, 0)
        tol2 = np.finfo(np.float64).eps ** 2
        r = self.residual0(b, x)
        rtilde = r.copy()
        rho_prev = omega = alpha = p = v = None
        tr = Trace(x, maxiter, maxiter, 0, rnorm0=self.norm(r))

        def leave(info, its, half):
            tr.info, tr.iterations, tr.half_step = info, its, half
            return tr

        for k in range(maxiter):
            if self.norm(r) < atol:
                return leave(0, k, 0)
            rho = self.rho(k, rtilde, r)
            if np.abs(rho) < tol2:
                return leave(-10, k, 0)
            if k > 0:
                if np.abs(omega) < tol2:
                    return leave(-11, k, 0)
                beta = self.beta(rho, rho_prev, alpha, omega)
                self.update_p(p, r, v, beta, omega)
            else:
                p = r.copy()
            phat = self.psolve(k, "p", p)
            v = self.A(phat)
            rv = self.dot(rtilde, v)
            if rv == 0:
                return leave(-11, k, 0)
            alpha = rho / rv
            tr.alpha.append(alpha)
            tr.rho.append(rho)
            r -= alpha * v          # s, in place
            tr.snorm.append(self.norm(r))
            if tr.snorm[-1] < atol:
                self.half_x(x, tr.alpha, phat)
                tr.omega.append(None)
                tr.xs.append(x.copy())
                tr.rs.append(r.copy())
                return leave(0, k + 1, 1)
            shat = self.psolve(k, "s", r)
            t = self.A(shat)
            omega = self.omega(t, r)
            tr.omega.append(omega)
            self.update_x(x, alpha, phat, omega, shat)
            r -= omega * t
            rho_prev = rho
            tr.xs.append(x.copy())
            tr.rs.append(r.copy())
        return tr


# ---------------------------------------------------------------------------------------
# the operators in both precisions
# ---------------------------------------------------------------------------------------
class _WithMinv:
    """A of an Operator, M^-1 a callable."""

    def __init__(self, base, minv):
        self.base, self.n, self.dtype = base, base.n, base.dtype
        self.A, self.Minv = base.A, (lambda r: minv(np.asarray(r).astype(base.dtype)))


@dataclass
class Ops:
    f64: object
    ld: object

    def of(self, dtype):
        return self.ld if dtype is LD else self.f64


def operators(indptr, indices, data, n, prec=None) -> Ops:
    """prec: None | ("bj", bs) | ("line", stride, seg) (oracle.arnoldi.Operator's own M^-1), or a
    pair of callables (M^-1 in float64, M^-1 in longdouble) for any other preconditioner."""
    if prec is not None and callable(prec[0]):
        return Ops(*(_WithMinv(Operator(indptr, indices, data, n, None, dt), m)
                     for dt, m in ((np.float64, prec[0]), (LD, prec[1]))))
    return Ops(Operator(indptr, indices, data, n, prec, np.float64), Operator(indptr, indices, data, n, prec, LD))


# ---------------------------------------------------------------------------------------
# the figure and the reference
# ---------------------------------------------------------------------------------------
def _nrm(v):
    return np.sqrt(v @ v)


def figure(x, x_ld) -> float:
    x_ld = np.asarray(x_ld).astype(LD)
    return float(_nrm(np.asarray(x).astype(LD) - x_ld) / _nrm(x_ld))


def run(ops: Ops, b, x0=None, *, dtype=LD, dot=np.dot, loop=Loop, **kw) -> Trace:
    o = ops.of(dtype)
    return loop(o.A, o.Minv, dtype, dot).solve(b, x0, **kw)


def reference(ops: Ops, b, x0, dots, *, maxiter, rtol=0.0, atol=0.0):
    """(the longdouble Trace, R): R[j] = max over ``dots`` of the float64 instance's figure of xs[j],
    floored at U.  The float64 runs must take the longdouble run's exit."""
    ld = run(ops, b, x0, maxiter=maxiter, rtol=rtol, atol=atol)
    R = [U] * len(ld.xs)
    for dot in dots:
        f = run(ops, b, x0, dtype=np.float64, dot=dot, maxiter=maxiter, rtol=rtol, atol=atol)
        assert (f.info, f.iterations, f.half_step) == (ld.info, ld.iterations, ld.half_step), \
            "the float64 instance left elsewhere than the longdouble reference"
        R = [max(Rj, figure(xj, lj)) for Rj, xj, lj in zip(R, f.xs, ld.xs)]
    return ld, R
