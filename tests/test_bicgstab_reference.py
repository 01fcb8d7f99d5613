"""The BiCGStab reference (oracle/bicgstab.py) checked on itself, without a GPU: the float64
instance is the NumPy twin of scipy.sparse.linalg.bicgstab bit for bit (tests/test_bicgstab_host.py
pins that twin to SciPy); for every case of tests/test_gpu_bicgstab_steps.py the reference figure
R_k (the float64 instance's own ||x_k - x_k^LD|| / ||x_k^LD||, the worst of three summation orders
of its dots, floored at 2^-53) keeps the device bar 16 R_k at or under 1e-12 for k = 1, 2, 3; every
planted defect -- of the size a misplaced beta, a stale scalar, a wrong lane or a dropped row would
have -- lifts the figure to at least ten times that bar at some k <= 3 (one entry of shat off by
1e-9: wherever its effect on x is that large); and the half-step cases leave where
the longdouble run leaves under every summation order.

The cases of the GPU module are defined here (CASES, HALF, RANKS) so that both modules read the
same list and the same cached references.
"""
import functools

import numpy as np
import pytest

from oracle import bicgstab as bc
from oracle import coracle, twin
from test_bicgstab_host import bicgstab_twin, dot_running, dot_strided, general_csr

LD = bc.LD
U = bc.U
MARGIN = 16.0
KMAX = 3
DOTS = (np.dot, dot_strided, dot_running)
SHARP = 1e-12           # the condition that keeps the GPU test sharp: 16 R_k <= SHARP
X0_SCALE, X0_SEED = 1e-3, 3

V7 = twin.Vlasov(2, (7, 24))      # n = 168: no multiple of 64, a partial last workgroup
GRID_OPS = ("S2", "S4", "S4F", "C0")
GRID_PRECS = ("none", "bj8", "bj4", "bj2", "bj1", "bj16", "line")
# beyond the grid: operator -> reference preconditioners ("line:2": S4's x-lines in segments of 2,
# the three-rank M)
EXTRA = {"S4": ("product", "cyclic", "line:2"), "S2": ("cyclic", "neumann"), "V7": ("bj8", "none"), "G": ("none", "bj8")}
CASES = [(name, prec, x0) for name in GRID_OPS for prec in GRID_PRECS for x0 in (0, 1)]
CASES += [(name, prec, x0) for name, precs in EXTRA.items() for prec in precs for x0 in (0, 1)]
# the half-step cases: (operator, preconditioner, x0) -> the iteration that leaves through ||s|| < atol
# (||s_k|| <= ||r_{k-1}|| / 4 there; S2 / line leaves so naturally; C0 / BJ(8): the fused M s of k_bcg_s)
HALF = {("S2", "line", 0): 1, ("S2", "line", 1): 3, ("S2", "cyclic", 0): 2, ("C0", "bj8", 0): 3}
# host-staged ranks: (operator, world) -> reference preconditioner
RANKS = {("S2", 2): "bj8", ("S2", 3): "bj8", ("S4", 2): "line", ("S4", 3): "line:2"}


def params_of(name):
    return V7 if name == "V7" else twin.CONFIGS[name]


def line_geometry(p):
    """tests/test_gpu_bicgstab.py's: (stride, segment) of the x-lines."""
    if p.dim == 1:
        return 1, 25
    if p.dim == 2:
        return p.shape[1], 25
    return p.shape[1] * p.shape[2] * p.shape[3], 3


def product_geometry(p):
    """tests/test_gpu_line_product.py's BiCGStab case: x-lines in segments of 3, y-lines of 5."""
    return (p.shape[1] * p.shape[2] * p.shape[3], 3), (p.shape[2] * p.shape[3], 5)


def cyclic_geometry(p):
    """(stride, period, seg): S2's x-lines (tests/test_gpu_line_cyclic.py, seg 25), S4's y-lines (seg 2)."""
    if p.dim == 2:
        return p.shape[1], p.shape[0], 25
    return p.shape[2] * p.shape[3], p.shape[1], 2


@functools.lru_cache(maxsize=None)
def system(name):
    """((indptr, indices, data), n, b), read-only.  "G": tests/test_bicgstab_host.py's general CSR."""
    if name == "G":
        R = general_csr()
        csr = (R.indptr.astype(np.int32), R.indices.astype(np.int32), R.data.copy())
        n = R.shape[0]
    else:
        p = params_of(name)
        csr, n = coracle.generate(p), p.n
    b = twin.rhs(n)
    for a in csr + (b,):
        a.setflags(write=False)
    return csr, n, b


@functools.lru_cache(maxsize=None)
def x0_of(name, flag):
    if not flag:
        return None
    x0 = X0_SCALE * twin.rhs(system(name)[1], seed=X0_SEED)
    x0.setflags(write=False)
    return x0


@functools.lru_cache(maxsize=None)
def ops(name, prec):
    """A and M^-1 in float64 and longdouble.  The product, cyclic and Neumann M^-1 are the
    references their own GPU modules pin an Arnoldi cycle with, passed in as callables."""
    (ip, ix, d), n, _ = system(name)
    if prec == "none":
        return bc.operators(ip, ix, d, n)
    if prec.startswith("bj"):
        return bc.operators(ip, ix, d, n, ("bj", int(prec[2:])))
    p = params_of(name)
    if prec.startswith("line"):
        stride, seg = line_geometry(p)
        return bc.operators(ip, ix, d, n, ("line", stride, int(prec[5:]) if ":" in prec else seg))
    if prec == "product":
        from test_gpu_line_product import ProductOperator
        make = lambda dt: ProductOperator(ip, ix, d, n, *product_geometry(p), dt)
    elif prec == "cyclic":
        from test_gpu_line_cyclic import CyclicOperator
        stride, period, _ = cyclic_geometry(p)
        make = lambda dt: CyclicOperator(ip, ix, d, n, stride, period, dt)
    elif prec == "neumann":
        from test_gpu_neumann import NeumannOperator
        make = lambda dt: NeumannOperator(ip, ix, d, n, 8, 2, dt)
    else:
        raise KeyError(prec)
    return bc.operators(ip, ix, d, n, (make(np.float64).Minv, make(LD).Minv))


@functools.lru_cache(maxsize=None)
def reference(name, prec, x0):
    """(longdouble Trace of KMAX iterations, [R_1, R_2, R_3]); computed once, never written to."""
    return bc.reference(ops(name, prec), system(name)[2], x0_of(name, x0), DOTS, maxiter=KMAX)


def half_atol(name, prec, x0):
    """(k, atol) of a half-step case: the geometric middle of 2 ||s_k|| <= atol <= ||r_{k-1}|| / 2 in
    the longdouble run, so that no summation order can move the exit (rtol = 0)."""
    k = HALF[(name, prec, x0)]
    ld, _ = reference(name, prec, x0)
    s_k = ld.snorm[k - 1]
    r_prev = ld.rnorm0 if k == 1 else np.sqrt(ld.rs[k - 2] @ ld.rs[k - 2])
    atol = float(np.sqrt(2 * s_k * (r_prev / 2)))
    assert 2 * s_k <= atol <= r_prev / 2, (float(s_k), atol, float(r_prev))
    # nothing before it leaves: every earlier ||r|| and ||s|| is at least twice atol
    before = [ld.rnorm0] + [np.sqrt(r @ r) for r in ld.rs[:k - 1]] + list(ld.snorm[:k - 1])
    assert min(before) >= 2 * atol, ([float(v) for v in before], atol)
    return k, atol


@functools.lru_cache(maxsize=None)
def half_reference(name, prec, x0):
    """(k, atol, longdouble Trace, R) of a half-step case; the float64 instance leaves at the same k
    through the half step under all three dot orders (asserted in bc.reference)."""
    k, atol = half_atol(name, prec, x0)
    ld, R = bc.reference(ops(name, prec), system(name)[2], x0_of(name, x0), DOTS, maxiter=KMAX, atol=atol)
    return k, atol, ld, R


def case_id(c):
    return f"{c[0]}-{c[1]}-x0{c[2]}"


# ---- 1. the float64 instance is the twin, bit for bit ------------------------------------------

class _Matmul:
    def __init__(self, mv):
        self.mv = mv

    def __matmul__(self, x):
        return self.mv(x)


@pytest.mark.parametrize("x0", [0, 1])
@pytest.mark.parametrize("prec", ["none", "bj8", "line"])
@pytest.mark.parametrize("name", ["S2", "S4", "C0"])
def test_float64_instance_is_the_twin(name, prec, x0):
    o = ops(name, prec).f64
    b = system(name)[2]
    for maxiter in (1, 2, 3):
        xt, infot, itst, halft = bicgstab_twin(_Matmul(o.A), b, x0_of(name, x0), rtol=0.0, maxiter=maxiter, M=o.Minv)
        tr = bc.run(ops(name, prec), b, x0_of(name, x0), dtype=np.float64, maxiter=maxiter)
        assert (tr.info, tr.iterations, tr.half_step) == (infot, itst, halft) == (maxiter, maxiter, 0)
        assert np.array_equal(tr.x, xt) and np.array_equal(tr.xs[-1], xt)
    # and through an exit: the twin's own tolerance test
    xt, infot, itst, halft = bicgstab_twin(_Matmul(o.A), b, x0_of(name, x0), rtol=1e-5, maxiter=200, M=o.Minv)
    tr = bc.run(ops(name, prec), b, x0_of(name, x0), dtype=np.float64, rtol=1e-5, maxiter=200)
    assert (tr.info, tr.iterations, tr.half_step) == (infot, itst, halft) and infot == 0
    assert np.array_equal(tr.x, xt)


# ---- 2. the bars stay sharp ---------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bars_are_sharp(case):
    ld, R = reference(*case)
    assert (ld.info, ld.iterations, ld.half_step) == (KMAX, KMAX, 0) and len(R) == KMAX
    print(f"BCG-REF|{case_id(case)}|" + "|".join(f"R_{k + 1} {r:.3e}" for k, r in enumerate(R)))
    for k, r in enumerate(R):
        assert r >= U and MARGIN * r <= SHARP, (k + 1, r)


def test_every_rank_case_is_a_case():
    for (name, world), prec in RANKS.items():
        assert (name, prec, 0) in CASES


# ---- 3. planted defects -------------------------------------------------------------------------

def _row(n):
    return (2 * n) // 3 + 1


class BetaBeforeSubtraction(bc.Loop):
    """p = r + beta p - omega v."""
    def update_p(self, p, r, v, beta, omega):
        p *= beta
        p -= omega * v
        p += r


class OmegaOverSS(bc.Loop):
    """omega = <t, s> / <s, s>."""
    def omega(self, t, s):
        return self.dot(t, s) / self.dot(s, s)


class BetaWithoutAlphaOverOmega(bc.Loop):
    def beta(self, rho, rho_prev, alpha, omega):
        return rho / rho_prev


class RhoFromR(bc.Loop):
    """rho = <r, r> for k >= 1."""
    def rho(self, k, rtilde, r):
        return self.dot(r, r) if k >= 1 else self.dot(rtilde, r)


class ShatEntryScaled(bc.Loop):
    """One entry of shat scaled by 1 + 1e-9 at iteration 2."""
    def psolve(self, k, which, y):
        z = self.Minv(y)
        if (k, which) == (1, "s"):
            z = z.copy()
            z[_row(len(z))] *= 1 + 1e-9
        return z


class PhatBlockRotated(bc.Loop):
    """One 8-row block's phat rotated by one row (every iteration)."""
    def psolve(self, k, which, y):
        z = self.Minv(y)
        if which == "p":
            z = z.copy()
            i = 8 * (_row(len(z)) // 8)
            z[i:i + 8] = np.roll(z[i:i + 8], 1)
        return z


class XRowWithoutOmegaShat(bc.Loop):
    """x without its omega shat term on one row."""
    def update_x(self, x, alpha, phat, omega, shat):
        i = _row(len(x))
        keep = x[i] + alpha * phat[i]
        x += alpha * phat
        x += omega * shat
        x[i] = keep


class HalfStepPreviousAlpha(bc.Loop):
    """The half-step exit with the previous iteration's alpha (none yet at iteration 1: zero)."""
    def half_x(self, x, alphas, phat):
        x += (alphas[-2] if len(alphas) > 1 else 0 * alphas[-1]) * phat


class R0IsB(bc.Loop):
    """r0 = b although x0 != 0."""
    def residual0(self, b, x):
        return b.copy()


DEFECTS = [BetaBeforeSubtraction, OmegaOverSS, BetaWithoutAlphaOverOmega, RhoFromR, ShatEntryScaled, PhatBlockRotated,
           XRowWithoutOmegaShat]


def _worst_ratio(tr, ld, R):
    """max over k of figure_k / (16 R_k): >= 10 is ten times the bar."""
    return max(bc.figure(x, xl) / (MARGIN * r) for x, xl, r in zip(tr.xs, ld.xs, R))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_planted_defects_are_seen(case):
    """Each defect, planted into the float64 instance, lifts the figure at some k <= 3 to at least
    10 x the bar (160 R_k); R0IsB where x0 != 0.

    The one exception is the test's reach, not a tolerance: ShatEntryScaled changes
    x_2 by 1e-9 |omega shat_i| / ||x||, and where the second correction is already small (S2 with
    the line preconditioners, the general CSR with BJ(8)) that is under 160 R_2 -- on S2 with the
    cyclic lines under the rounding of x itself.  Its exact size is measured by planting it into
    the longdouble instance; it must be seen wherever that size is at least 20 x the bar."""
    name, prec, x0 = case
    ld, R = reference(*case)
    args = (ops(name, prec), system(name)[2], x0_of(name, x0))
    clean = bc.run(*args, dtype=np.float64, maxiter=KMAX)
    assert _worst_ratio(clean, ld, R) <= 1 / MARGIN
    bad = []
    for D in DEFECTS + ([R0IsB] if x0 else []):
        ratio = _worst_ratio(bc.run(*args, dtype=np.float64, maxiter=KMAX, loop=D), ld, R)
        size = _worst_ratio(bc.run(*args, maxiter=KMAX, loop=D), ld, R) if D is ShatEntryScaled else np.inf
        print(f"BCG-DEFECT|{case_id(case)}|{D.__name__}|figure / bar x{ratio:.3g}" +
              (f"|exact size / bar x{size:.3g}" if D is ShatEntryScaled else ""))
        if size >= 20 and not ratio >= 10:
            bad.append((D.__name__, ratio))
    assert not bad, bad


# ---- 4. the half-step cases ---------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(HALF), ids=case_id)
def test_half_step_cases(case):
    """An atol inside 2 ||s_k|| <= atol <= ||r_{k-1}|| / 2 of the longdouble run with rtol = 0: the
    float64 instance leaves at the same k through the half step under all three dot orders
    (bc.reference asserts it), the bar stays sharp, and the exit with the previous alpha is seen."""
    name, prec, x0 = case
    k, atol, ld, R = half_reference(*case)
    assert (ld.info, ld.iterations, ld.half_step) == (0, k, 1) and len(ld.xs) == k == HALF[case] <= KMAX
    print(f"BCG-HALF|{case_id(case)}|k {k}|atol {atol:.3e}|" + "|".join(f"R_{j + 1} {r:.3e}" for j, r in enumerate(R)))
    for r in R:
        assert MARGIN * r <= SHARP, r
    tr = bc.run(ops(name, prec), system(name)[2], x0_of(name, x0), dtype=np.float64, maxiter=KMAX, atol=atol,
                loop=HalfStepPreviousAlpha)
    assert (tr.iterations, tr.half_step) == (k, 1)
    ratio = bc.figure(tr.x, ld.x) / (MARGIN * R[-1])
    print(f"BCG-DEFECT|{case_id(case)}|HalfStepPreviousAlpha|figure / bar x{ratio:.3g}")
    assert ratio >= 10, ratio
