"""The extended-precision Arnoldi reference (oracle/arnoldi.py) on the CPU: the longdouble run
satisfies its own figures at the 1e-19 level, the plain float64 CGS2 and MGS runs sit at float64
rounding (these are the figures the GPU bars in tests/test_gpu_arnoldi_steps.py are multiples
of), and each planted defect -- of the size a dropped row, a stale ghost line or a swapped
rotation would cause -- raises its figure at least 100x above the undisturbed value.

Figures: F1 the Arnoldi relation per column, F2 orthonormality, F3 the cycle
start (v_0 and beta), F4 the rotated H / rotations / S against a longdouble Givens QR of the raw
columns, F5 the x correction against the longdouble minimiser's, F6 the reported preconditioned
residual against the true one.
"""
import copy
import functools

import numpy as np
import pytest

from oracle import arnoldi as ar
from oracle import twin

K = 20
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _runs(name):
    p = twin.CONFIGS[name]
    ip, ix, d = twin.generate(p)
    b = twin.rhs(p.n)
    opl = ar.Operator(ip, ix, d, p.n, ("bj", 8))
    op64 = ar.Operator(ip, ix, d, p.n, ("bj", 8), np.float64)
    x0 = np.zeros(p.n)
    delta = ar.minimiser(opl, b, x0, K)
    out = {"p": p, "b": b, "opl": opl, "delta": delta}
    for scheme, op in (("cgs2x", opl), ("cgs2", op64), ("mgs", op64)):
        out[scheme] = ar.run_cycle(op, b, x0, K, scheme)
    return out


def _fig(r, cyc):
    return ar.worst(ar.figures(r["opl"], r["b"], cyc, r["delta"]))


def test_longdouble_is_extended():
    assert np.finfo(ar.LD).eps < 2e-19


def test_operator_matches_float64_oracle():
    """The longdouble operator is the same operator: A x and M^-1 r agree with the float64 NumPy
    oracle to float64 rounding; float32 values are widened, not re-derived."""
    for name in ("S2", "S4F"):
        p = twin.CONFIGS[name]
        ip, ix, d = twin.generate(p)
        op = ar.Operator(ip, ix, d, p.n, ("bj", 8))
        x = twin.rhs(p.n, seed=7)
        y = twin.scipy_csr(ip, ix, d.astype(np.float64), p.n) @ x
        assert np.max(np.abs(op.A(x).astype(np.float64) - y)) <= 8 * EPS * np.max(np.abs(y))
        z = twin.bj_apply_numpy(twin.bj_inverse_numpy(ip, ix, d, p.n, 8), x, p.n)
        assert np.max(np.abs(op.Minv(x).astype(np.float64) - z)) <= 64 * EPS * np.max(np.abs(z))
        assert np.array_equal(op.data.astype(d.dtype), d)
    p = twin.CONFIGS["S2"]
    ip, ix, d = twin.generate(p)
    for seg in (8, 25, 1 << 30):
        op = ar.Operator(ip, ix, d, p.n, ("line", p.shape[1], seg))
        x = twin.rhs(p.n, seed=9)
        z = twin.line_apply_numpy(twin.line_factors_numpy(ip, ix, d, p.n, p.shape[1], min(seg, p.shape[0])), x,
                                  p.shape[1], min(seg, p.shape[0]))
        assert np.max(np.abs(op.Minv(x).astype(np.float64) - z)) <= 64 * EPS * np.max(np.abs(z)), seg


@pytest.mark.parametrize("name", ["S2", "S4", "S4F"])
def test_reference_figures(name):
    r = _runs(name)
    f = _fig(r, r["cgs2x"])
    print(name, "longdouble", f)
    # the reference: two to three orders below float64 rounding everywhere (v_0 and the
    # correction are its own: 0; beta and the rotations pass through an un-rotation)
    assert f["F1"] < 2e-19 and f["F2"] < 1e-17 and f["F6"] < 1e-17, f
    assert f["F3b"] < 1e-18 and f["F4"] < 1e-18 and f["F3v"] == f["F5"] == 0.0, f
    c = _fig(r, r["cgs2"])
    m = _fig(r, r["mgs"])
    print(name, "float64 cgs2", c)
    print(name, "float64 mgs ", m)
    # float64 rounding: an eps or two per figure (measured 1.0e-16 .. 5.3e-16); F6 carries
    # beta / presid on top of the rounding of x (up to 1.8e-15).  MGS loses orthogonality in
    # proportion to the conditioning of [v_0, B V] (5e-14 .. 9e-14 here): no rounding-level bar
    for g in (c, m):
        assert g["F1"] < 2 * EPS and g["F3v"] < EPS and g["F3b"] < 2 * EPS and g["F5"] < 4 * EPS, g
        assert g["F6"] < 16 * EPS, g
    assert c["F2"] < 2 * EPS and c["F4"] < EPS, c
    assert 16 * EPS < m["F2"] < 1e-12, m


def _col_max(cyc, c):
    return int(np.argmax(np.abs(cyc.V[c])))


@pytest.mark.parametrize("name", ["S2", "S4", "S4F"])
def test_planted_defects_are_seen(name):
    r = _runs(name)
    base = _fig(r, r["cgs2"])
    p = r["p"]
    line = p.shape[-1]

    def plant(fn):
        cyc = copy.deepcopy(r["cgs2"])
        fn(cyc)
        return _fig(r, cyc)

    def scale_v(cyc):
        cyc.V[9, _col_max(cyc, 9)] *= 1 + 1e-9
    f = plant(scale_v)
    print(name, "v_9 entry * (1 + 1e-9):", f["F1"], f["F2"], "base", base["F1"], base["F2"])
    assert f["F1"] >= 100 * base["F1"] and f["F2"] >= 100 * base["F2"]

    def scale_h(cyc):
        cyc.Hraw[11, 3] *= 1 + 1e-10
    f = plant(scale_h)
    print(name, "h_{3,11} * (1 + 1e-10):", f["F1"], "base", base["F1"])
    assert f["F1"] >= 100 * base["F1"]

    def stale_line(cyc):
        cyc.V[9, 2 * line:3 * line] = cyc.V[8, 2 * line:3 * line]
    f = plant(stale_line)
    print(name, "v_9 line 2 from v_8:", f["F1"], f["F2"])
    assert f["F1"] >= 100 * base["F1"] and f["F2"] >= 100 * base["F2"]

    def swap_givens(cyc):
        cyc.giv[7] = cyc.giv[7][::-1].copy()
    f = plant(swap_givens)
    print(name, "(c_7, s_7) transposed:", f["F4"], "base", base["F4"])
    assert f["F4"] >= 100 * base["F4"]

    def drop_last(cyc):
        y = ar.hess_solve(cyc.H, cyc.S, K)
        cyc.x_out = cyc.x_out - y[K - 1] * cyc.V[K - 1]
    f = plant(drop_last)
    print(name, "x_out without the last column's term:", f["F5"], "base", base["F5"])
    assert f["F5"] >= 100 * base["F5"]


def test_mgs_columns_unrotate():
    """Under MGS only the rotated H survives: the raw column rebuilt from H and giv gives the same
    F1 as the raw column itself."""
    r = _runs("S2")
    op64 = ar.Operator(*twin.generate(r["p"]), r["p"].n, ("bj", 8), np.float64)
    V, Hraw = ar.arnoldi(op64, r["mgs"].V[0], K, "mgs")
    for c in (0, 7, K - 1):
        h = ar.unrotate_column(r["mgs"].H[c], r["mgs"].giv, c)
        assert np.max(np.abs(h - Hraw[c, :c + 2].astype(ar.LD))) <= 8 * EPS * np.max(np.abs(Hraw[c, :c + 2]))
