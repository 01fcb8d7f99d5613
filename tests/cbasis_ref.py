"""NumPy restatement of compressed-basis GMRES -- TEST INFRASTRUCTURE ONLY.

Left-preconditioned restarted GMRES under SciPy's control flow (scipy/sparse/linalg/_isolve/
iterative.py:692-841: the ptol test and its schedule -- or, ``schedule="fixed"``, the test against the
solve's first ptol in every cycle --, the dlartg rotations, the breakdown test, the true residual
at every restart) with a float64 CGS2 Arnoldi (two classical passes) whose columns are rounded to
float32 when they are stored: every later use of a column -- the projections, the x update -- sees
the stored value, every operation is float64.  ``basis="float64"`` stores the columns unrounded (the
same code, the counts the float32 basis is compared with).

Two variants of what the operator is applied to:
  ``"rounded"``    B v^_c, the stored column (the default of the functions below);
  ``"candidate"``  B u_c, the unrounded vector the column was rounded from -- what the delayed DCGS2
                   of the device does, whose candidate p_c stays float64: the variant a captured
                   device cycle is compared with (compare()).

The operator is an ``oracle.arnoldi.Operator`` in float64 (B = M^-1 A from the CSR as stored), so
block Jacobi, line Jacobi and no preconditioner are covered; one cycle comes back as the
``oracle.arnoldi.Cycle`` record that ``oracle.arnoldi.figures`` measures in 80-bit.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import arnoldi as ar

EPS = float(np.finfo(np.float64).eps)


def store(v, basis):
    """The column as the basis keeps it (float64 array; float32 basis: of float32 values)."""
    if basis == "float64":
        return np.array(v, np.float64)
    if basis == "float32":
        return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    raise ValueError(f"unknown basis {basis!r}")


def arnoldi_cb(op: ar.Operator, v0, k, basis="float32", variant="rounded", ptol=None, beta=None):
    """Up to k CGS2 columns from the unit vector v0.  Returns (V [cols + 1, n] as stored, Hraw
    [cols, k + 2], H rotated, giv, S, cols, presid, breakdown).  With ptol and beta the loop stops as
    SciPy's does (presid <= ptol, or h1 <= eps h0), else it runs all k columns."""
    assert op.dtype is np.float64 and variant in ("rounded", "candidate")
    n = op.n
    V = np.zeros((k + 1, n))
    Hraw = np.zeros((k, k + 2))
    H = np.zeros((k, k + 1))
    giv = np.zeros((k, 2))
    S = np.zeros(k + 1)
    S[0] = 1.0 if beta is None else beta
    V[0] = store(v0, basis)
    u = V[0].copy()     # the unrounded vector column c was stored from (c = 0: the operator takes the stored v^_0)
    cols, presid, breakdown = 0, 0.0, False
    for c in range(k):
        w = op.B(V[c] if variant == "rounded" else u)
        h0 = np.sqrt(w @ w)
        h = np.zeros(c + 1)
        for _ in range(2):
            t = V[:c + 1] @ w
            w = w - t @ V[:c + 1]
            h = h + t
        h1 = np.sqrt(w @ w)
        Hraw[c, :c + 1] = h
        Hraw[c, c + 1] = h1
        if h1 <= EPS * h0:
            Hraw[c, c + 1] = 0.0
            breakdown = True
            u = w
        else:
            u = w * (1.0 / h1)
        V[c + 1] = store(u, basis)
        # SciPy's rotations on column c (iterative.py:772-787)
        col = Hraw[c, :c + 2].copy()
        for j in range(c):
            cg, sg = giv[j]
            col[j], col[j + 1] = cg * col[j] + sg * col[j + 1], -sg * col[j] + cg * col[j + 1]
        cg, sg, r = ar.lartg(np.float64(col[c]), np.float64(col[c + 1]))
        giv[c] = cg, sg
        col[c], col[c + 1] = r, 0.0
        H[c, :c + 2] = col
        S[c], S[c + 1] = cg * S[c], -sg * S[c]
        cols = c + 1
        presid = abs(S[c + 1])
        if ptol is not None and (presid <= ptol or breakdown):
            break
    return V[:cols + 1], Hraw[:cols], H[:cols], giv[:cols], S[:cols + 1], cols, presid, breakdown


def run_cycle_cb(op: ar.Operator, b, x_in, k, basis="float32", variant="rounded") -> ar.Cycle:
    """One full cycle of k columns as the record oracle.arnoldi.figures reads."""
    x_in = np.asarray(x_in, np.float64)
    r0 = op.presidual(b, x_in)
    beta = np.sqrt(r0 @ r0)
    V, Hraw, H, giv, S, cols, presid, _ = arnoldi_cb(op, r0 * (1.0 / beta), k, basis, variant, beta=beta)
    y = ar.hess_solve(H, S, cols)
    x_out = x_in + y @ V[:cols]
    return ar.Cycle(V=V, cols=cols, final_cols=cols + 1, x_in=x_in, x_out=x_out, H=H, S=S, giv=giv,
                    presid=presid, Hraw=Hraw)


@dataclass
class CbSolve:
    x: np.ndarray
    info: int
    inner_iters: int
    cycles: int
    rnorm: float
    atol_eff: float
    history: list = field(default_factory=list)   # per cycle: (columns, presid, ptol, rnorm)


def solve_cb(op: ar.Operator, b, x0=None, *, rtol=1e-8, atol=0.0, restart=20, maxiter=None, basis="float32",
             variant="rounded", schedule="scipy") -> CbSolve:
    """scipy.sparse.linalg.gmres's loop around arnoldi_cb.  schedule: what the inner test
    presid <= ptol is held against from the second cycle on --
      "scipy"  SciPy's whole schedule: ptol = presid min(ptol_max_factor, atol / rnorm), re-derived at
               every restart (iterative.py:826-835) -- what the device runs;
      "fixed"  SciPy's ptol test against the solve's first ptol = ||M b|| min(1, atol / ||b||) in every
               cycle: the cycle that meets it is followed by cycles of one column until the true
               residual is under atol (S2 / BJ(8) at restart 20: 20, 20, 20, 6, 1, 1 against SciPy's
               20, 20, 20, 8).  The iteration table the compressed basis was argued with uses this one."""
    assert schedule in ("scipy", "fixed")
    b = np.asarray(b, np.float64)
    n = op.n
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64)
    maxiter = 10 * n if maxiter is None else maxiter
    restart = min(restart, n)
    bnrm2 = np.linalg.norm(b)
    atol = max(atol, rtol * bnrm2)
    if bnrm2 == 0.0:
        return CbSolve(b.copy(), 0, 0, 0, 0.0, atol)
    Mb = np.linalg.norm(op.Minv(b))
    ptol_max_factor = 1.0
    ptol = Mb * min(ptol_max_factor, atol / bnrm2)
    r = b - op.A(x) if x.any() else b.copy()
    rnorm = np.linalg.norm(r)
    out = CbSolve(x, 0, 0, 0, float(rnorm), float(atol))
    if rnorm < atol:
        return out
    for it in range(maxiter):
        z = op.Minv(r)
        beta = np.sqrt(z @ z)
        V, Hraw, H, giv, S, cols, presid, brk = arnoldi_cb(op, z * (1.0 / beta), restart, basis, variant, ptol, beta)
        S = S.copy()
        if H[cols - 1, cols - 1] == 0.0:
            S[cols - 1] = 0.0
        y = np.zeros(cols)
        for c in range(cols - 1, -1, -1):          # iterative.py:799-812
            if S[c] != 0.0:
                y[c] = S[c] / H[c, c]
                S[:c] = S[:c] - y[c] * H[c, :c]
        x = x + y @ V[:cols]
        r = b - op.A(x)
        rnorm = np.linalg.norm(r)
        out.inner_iters += cols
        out.cycles = it + 1
        out.history.append((cols, float(presid), float(ptol), float(rnorm)))
        if rnorm <= atol or brk:
            break
        if schedule == "fixed":
            continue
        if presid <= ptol:
            ptol_max_factor = max(EPS, 0.25 * ptol_max_factor)
        else:
            ptol_max_factor = min(1.0, 1.5 * ptol_max_factor)
        ptol = presid * min(ptol_max_factor, atol / rnorm)
    out.x, out.rnorm = x, float(rnorm)
    out.info = 0 if rnorm <= atol else maxiter
    return out


# ---------------------------------------------------------------------------------------
# operators beyond oracle.arnoldi's own kinds, in a chosen precision
# ---------------------------------------------------------------------------------------
def diag_sum(indptr, indices, data):
    """D[r]: row r's stored entries with col == row, summed in stored order from 0.0."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(indptr, np.int64)))
    m = np.asarray(indices, np.int64) == rows
    D = np.zeros(n)
    np.add.at(D, rows[m], np.asarray(data, np.float64)[m])
    return D


class ProductOperator(ar.Operator):
    """M^-1 r = M2^-1 (D (M1^-1 r)), M1 and M2 line operators (stride, seg) of oracle.arnoldi."""

    def __init__(self, indptr, indices, data, n, d1, d2, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        self.l1 = ar.Operator(indptr, indices, data, n, ("line",) + tuple(d1), dtype)
        self.l2 = ar.Operator(indptr, indices, data, n, ("line",) + tuple(d2), dtype)
        self.D = diag_sum(indptr, indices, data).astype(dtype)

    def Minv(self, r):
        return self.l2.Minv(self.D * self.l1.Minv(r))


class NeumannOperator(ar.Operator):
    """N_k^-1 r: z = M^-1 r, then k - 1 corrections z + M^-1 (r - A z), M block Jacobi."""

    def __init__(self, indptr, indices, data, n, bs, degree, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        self.base = ar.Operator(indptr, indices, data, n, ("bj", bs), dtype)
        self.degree = degree

    def Minv(self, r):
        r = np.asarray(r).astype(self.dtype)
        z = self.base.Minv(r)
        for _ in range(self.degree - 1):
            z = z + self.base.Minv(r - self.A(z))
        return z


class CyclicOperator(ar.Operator):
    """M: A's diagonal and its couplings along whole periodic lines (element i of line (block, j) at
    row (block period + i) stride + j, coupled to i +- 1 modulo period); every line's dense system
    inverted by oracle.arnoldi's pivoted Gauss-Jordan in the chosen precision."""

    def __init__(self, indptr, indices, data, n, stride, period, dtype=ar.LD):
        super().__init__(indptr, indices, data, n, None, dtype)
        assert n % (stride * period) == 0
        self.stride, self.period = stride, period
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.indptr))
        cols = self.indices
        line = lambda R: (R // (stride * period)) * stride + R % stride
        pos = lambda R: (R // stride) % period
        d = (pos(cols) - pos(rows)) % period
        keep = (line(rows) == line(cols)) & ((d == 0) | (d == 1) | (d == period - 1))
        B = np.zeros((n // period, period, period), dtype)
        np.add.at(B, (line(rows)[keep], pos(rows)[keep], pos(cols)[keep]), self.data[keep])
        self.inv = ar._gauss_inverse(B)

    def Minv(self, r):
        s, P = self.stride, self.period
        r = np.asarray(r).astype(self.dtype).reshape(-1, P, s)              # [block, i, j]
        rl = np.transpose(r, (0, 2, 1)).reshape(-1, P, 1)                   # [line, i]
        z = np.matmul(self.inv, rl).reshape(-1, s, P)
        return np.transpose(z, (0, 2, 1)).reshape(-1)


class Ops:
    """The longdouble and float64 forms of one preconditioned operator.  kind: None | ("bj", bs) |
    ("line", stride, seg) | ("product", d1, d2) | ("cyclic", stride, period) | ("neumann", bs, degree)"""

    def __init__(self, csr, n, kind):
        ip, ix, d = csr

        def make(dtype):
            if kind is None or kind[0] in ("bj", "line"):
                return ar.Operator(ip, ix, d, n, kind, dtype)
            cls = {"product": ProductOperator, "cyclic": CyclicOperator, "neumann": NeumannOperator}[kind[0]]
            return cls(ip, ix, d, n, *kind[1:], dtype=dtype)
        self.n, self.ld, self.f64 = n, make(ar.LD), make(np.float64)


# ---------------------------------------------------------------------------------------
# the bars of a captured compressed-basis cycle
# ---------------------------------------------------------------------------------------
MARGIN = 16.0           # what the project grants a device Arnoldi step over the plain float64 one
U = 2.0 ** -53
DEFECT_CAP = 5.2e-14    # tests/test_gpu_arnoldi_steps.py: no floor lifts a bar above it


# The device's delayed DCGS2 keeps its candidate p_c in float64 and applies the operator to it
# (include/vtkrylov.h, "compressed Krylov basis"), so "the restatement of the same case" is the
# candidate variant.  The two variants are different algorithms at the float32 level: the stored
# column's Arnoldi relation carries B (u_c - v^_c) in one and h_{c+1,c} (u_{c+1} - v^_{c+1}) in the
# other, and where h_{c+1,c} << ||B|| (the outlier operator's columns, the line preconditioners) the
# rounded variant's F1 and F6 are up to 30x below the candidate variant's own (R, n = 1026, 24
# columns: F6 1.2e-7 against 1.6e-6; tests/test_cbasis_host.py records both).
DEVICE_VARIANT = "candidate"


def compare(tag, ops: Ops, b, cyc: ar.Cycle, which=("F1", "F2", "F3v", "F3b", "F4", "F4e", "F5", "F6"), out=None):
    """F1-F6 of a device cycle (80-bit, oracle.arnoldi.figures) against the same figures of this
    module's float32-basis cycle (DEVICE_VARIANT) on the same operator, x_in and column count: each at most MARGIN
    times the restatement's.  F3b and F6, errors of one float64 scalar, take their reference no lower
    than the format allows (the floors of tests/test_gpu_arnoldi_steps.py, which only ever raise a
    reference that fell below the unit roundoff).  Every figure is printed before it is asserted."""
    delta = ar.minimiser(ops.ld, b, cyc.x_in, cyc.cols)
    fd = ar.figures(ops.ld, b, cyc, delta)
    dev = ar.worst(fd)
    ref = ar.worst(ar.figures(ops.ld, b, run_cycle_cb(ops.f64, b, cyc.x_in, cyc.cols, variant=DEVICE_VARIANT), delta))
    if cyc.early:
        dev["F4e"] = max(fd["F4"][c] for c in cyc.early)
        dev["F4"] = max([f for c, f in enumerate(fd["F4"]) if c not in cyc.early], default=0.0)
        ref["F4e"] = ref["F4"]
    xin = np.asarray(cyc.x_in).astype(ar.LD)
    r_in, r_out = ops.ld.presidual(b, xin), ops.ld.presidual(b, xin + delta)
    amp = float(np.sqrt(r_in @ r_in) / np.sqrt(r_out @ r_out))
    floor = {"F3b": U, "F6": min(U * amp, DEFECT_CAP / MARGIN)}
    bad = []
    for k in which:
        if k not in dev:
            continue
        r_eff = max(ref[k], floor.get(k, 0.0))
        ratio = dev[k] / r_eff if r_eff > 0 else (0.0 if dev[k] == 0 else np.inf)
        print(f"CB|{tag}|k={cyc.cols} fin={cyc.final_cols}|{k}|dev {dev[k]:.3e}|ref {ref[k]:.3e}|x{ratio:.2f}")
        if out is not None:
            out[k] = max(out.get(k, 0.0), ratio)
        if not dev[k] <= MARGIN * r_eff:
            bad.append((k, dev[k], ref[k], ratio))
    assert not bad, (tag, bad)
    return dev, ref


def cycle_of(cap, x_out, presid) -> ar.Cycle:
    """A device capture (vtkrylov.ArnoldiCapture) as the record the figures read."""
    early = {}
    if cap.Hraw is not None and cap.xup_tag >= 0 and cap.xup_tag == cap.stop_col:
        early[cap.stop_col] = cap.nu      # the stop column was committed from its tentative form
    return ar.Cycle(V=cap.V, cols=cap.cols, final_cols=cap.final_cols, x_in=cap.x_in, x_out=x_out, H=cap.H,
                    S=cap.S, giv=cap.giv, presid=presid, Hraw=cap.Hraw, early=early)
