"""Extended-precision reference for ONE restart cycle of preconditioned GMRES -- TEST
INFRASTRUCTURE ONLY (NumPy; nothing in the product imports it).

The solve-level bars (same info, inner iterations +-1, x to 1e-9) cannot see an Arnoldi step
that is wrong at the 1e-12 level: restarted GMRES repairs it in the next cycle.  This module
states what one cycle has to satisfy, in ``np.longdouble`` (x87 80-bit, eps 1.08e-19), so that a
captured cycle (``vtkrylov.last_arnoldi``) -- or any float64 Arnoldi -- can be measured against
it column by column:

* :class:`Operator`: B = M^-1 A from the CSR values as stored (float32 values widened), A a
  longdouble CSR product, M^-1 a batched longdouble Gaussian elimination on A's own diagonal
  blocks (block Jacobi), the longdouble Thomas solve of ``twin.line_matrix`` (line Jacobi) or I.
* :func:`arnoldi`: Arnoldi in a chosen precision; ``"cgs2x"`` (two full classical passes, the
  longdouble reference), ``"cgs2"`` and ``"mgs"`` (the plain float64 implementations whose
  rounding level sets the bars).
* :func:`run_cycle`: one GMRES cycle of k columns in a chosen precision as a :class:`Cycle`,
  the same record a device capture is turned into.
* :func:`figures`: F1-F6 of DESIGN.md §5, all evaluated in longdouble.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import twin

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "oracle.arnoldi needs an extended-precision np.longdouble (x87 80-bit)"


# ---------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------
def _gauss_inverse(B):
    """Batched Gauss-Jordan inverse with partial pivoting, in B's dtype.  B: [nb, bs, bs]."""
    nb, bs, _ = B.shape
    A = B.copy()
    X = np.zeros_like(A)
    X[:, np.arange(bs), np.arange(bs)] = 1
    idx = np.arange(nb)
    for k in range(bs):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        for M in (A, X):
            rk, rp = M[idx, k].copy(), M[idx, p].copy()
            M[idx, k], M[idx, p] = rp, rk
        piv = A[:, k, k].copy()
        if np.any(piv == 0):
            raise np.linalg.LinAlgError("singular diagonal block")
        A[:, k] = A[:, k] / piv[:, None]
        X[:, k] = X[:, k] / piv[:, None]
        for i in range(bs):
            if i != k:
                f = A[:, i, k].copy()
                A[:, i] = A[:, i] - f[:, None] * A[:, k]
                X[:, i] = X[:, i] - f[:, None] * X[:, k]
    return X


class Operator:
    """B = M^-1 A in ``dtype`` (longdouble: the reference; float64: the plain implementation).

    prec: None | ("bj", bs) | ("line", stride, seg)"""

    def __init__(self, indptr, indices, data, n, prec=None, dtype=LD):
        self.n, self.dtype, self.prec = int(n), dtype, prec
        self.indptr = np.asarray(indptr, np.int64)
        self.indices = np.asarray(indices, np.int64)
        self.data = np.asarray(data).astype(dtype)          # float32 values widen exactly
        assert np.all(np.diff(self.indptr) > 0), "empty rows are not supported (reduceat)"
        if prec is None:
            self.kind = "none"
        elif prec[0] == "bj":
            self.kind, self.bs = "bj", int(prec[1])
            blocks = twin.bj_blocks(indptr, indices, np.zeros(len(self.data)), n, self.bs).astype(dtype)
            rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.indptr))
            m = (self.indices // self.bs) == (rows // self.bs)
            np.add.at(blocks, (rows[m] // self.bs, rows[m] % self.bs, self.indices[m] % self.bs), self.data[m])
            self.inv = _gauss_inverse(blocks)
        elif prec[0] == "line":
            self.kind, self.stride = "line", int(prec[1])
            seg = int(min(prec[2], 1 << 40))
            M = twin.line_matrix(indptr, indices, np.asarray(data, np.float64), n, self.stride, seg)
            s = self.stride
            self.lb = M.diagonal(0).astype(dtype)
            self.la = np.concatenate([np.zeros(s), M.diagonal(-s)]).astype(dtype)   # a[r]: M[r, r - s]
            self.lc = np.concatenate([M.diagonal(s), np.zeros(s)]).astype(dtype)    # c[r]: M[r, r + s]
            assert n % s == 0
        else:
            raise ValueError(prec)

    def A(self, x):
        x = np.asarray(x).astype(self.dtype)
        return np.add.reduceat(self.data * x[self.indices], self.indptr[:-1])

    def Minv(self, r):
        r = np.asarray(r).astype(self.dtype)
        if self.kind == "none":
            return r.copy()
        if self.kind == "bj":
            nb = self.inv.shape[0]
            rp = np.zeros(nb * self.bs, self.dtype)
            rp[:self.n] = r
            return np.matmul(self.inv, rp.reshape(nb, self.bs, 1)).reshape(-1)[:self.n]
        s, X = self.stride, self.n // self.stride
        a, b, c = (v.reshape(X, s) for v in (self.la, self.lb, self.lc))
        d = r.reshape(X, s).copy()
        u = b.copy()
        for i in range(1, X):                      # Thomas; a = 0 at a segment's first line
            w = a[i] / u[i - 1]
            u[i] = b[i] - w * c[i - 1]
            d[i] = d[i] - w * d[i - 1]
        z = d
        z[X - 1] = d[X - 1] / u[X - 1]
        for i in range(X - 2, -1, -1):
            z[i] = (d[i] - c[i] * z[i + 1]) / u[i]
        return z.reshape(-1)

    def B(self, v):
        return self.Minv(self.A(v))

    def presidual(self, b, x):
        return self.Minv(np.asarray(b).astype(self.dtype) - self.A(x))


# ---------------------------------------------------------------------------------------
# Givens QR with LAPACK 3.10 dlartg's conventions (the lartg SciPy's gmres calls)
# ---------------------------------------------------------------------------------------
def lartg(f, g):
    dt = type(f)
    if g == 0:
        return dt(1), dt(0), f
    if f == 0:
        return dt(0), np.copysign(dt(1), g), abs(g)
    d = np.sqrt(f * f + g * g)
    c = abs(f) / d
    r = np.copysign(d, f)
    return c, g / r, r


def givens_qr(Hraw, beta, k):
    """Rotate the first k columns of the raw Hessenberg (Hraw[c, :c+2] = column c) as SciPy does.
    Returns (H rotated [k, k+1], giv [k, 2], S [k+1]) in Hraw's dtype."""
    dt = Hraw.dtype.type
    H = np.zeros((k, k + 1), Hraw.dtype)
    giv = np.zeros((k, 2), Hraw.dtype)
    S = np.zeros(k + 1, Hraw.dtype)
    S[0] = beta
    for c in range(k):
        h = Hraw[c, :c + 2].copy()
        for j in range(c):
            cg, sg = giv[j]
            h[j], h[j + 1] = cg * h[j] + sg * h[j + 1], -sg * h[j] + cg * h[j + 1]
        cg, sg, r = lartg(dt(h[c]), dt(h[c + 1]))
        giv[c] = cg, sg
        h[c], h[c + 1] = r, 0
        H[c, :c + 2] = h
        S[c], S[c + 1] = cg * S[c], -sg * S[c]
    return H, giv, S


def unrotate_column(hc, giv, c):
    """The raw column c (rows 0..c+1) from its rotated form and the rotations 0..c."""
    h = np.asarray(hc[:c + 2]).astype(LD).copy()
    for j in range(c, -1, -1):
        cg, sg = LD(giv[j][0]), LD(giv[j][1])
        h[j], h[j + 1] = cg * h[j] - sg * h[j + 1], sg * h[j] + cg * h[j + 1]
    return h


def unrotate_S(S, giv, k):
    s = np.asarray(S[:k + 1]).astype(LD).copy()
    for j in range(k - 1, -1, -1):
        cg, sg = LD(giv[j][0]), LD(giv[j][1])
        s[j], s[j + 1] = cg * s[j] - sg * s[j + 1], sg * s[j] + cg * s[j + 1]
    return s


def hess_solve(H, S, k):
    """y of the rotated least squares: back substitution on the k leading rotated columns."""
    y = np.asarray(S[:k]).copy()
    for c in range(k - 1, -1, -1):
        y[c] = y[c] / H[c, c]
        y[:c] = y[:c] - y[c] * H[c, :c]
    return y


# ---------------------------------------------------------------------------------------
# Arnoldi and one GMRES cycle
# ---------------------------------------------------------------------------------------
def arnoldi(op: Operator, v0, k, scheme):
    """k Arnoldi columns from the unit vector v0, in op.dtype.  Returns V [k+1, n] (row c = v_c) and
    Hraw [k, k+2] (Hraw[c, :c+2] = column c).  scheme: "mgs" (SciPy's loop), "cgs2" (classical,
    one re-orthogonalisation pass), "cgs2x" (two full re-orthogonalisation passes)."""
    dt = op.dtype
    V = np.zeros((k + 1, op.n), dt)
    Hraw = np.zeros((k, k + 2), dt)
    V[0] = v0
    for c in range(k):
        w = op.B(V[c])
        h = np.zeros(c + 1, dt)
        if scheme == "mgs":
            for j in range(c + 1):
                h[j] = V[j] @ w
                w = w - h[j] * V[j]
        else:
            for _ in range(3 if scheme == "cgs2x" else 2):
                t = V[:c + 1] @ w
                w = w - t @ V[:c + 1]
                h = h + t
        nrm = np.sqrt(w @ w)
        Hraw[c, :c + 1] = h
        Hraw[c, c + 1] = nrm
        V[c + 1] = w / nrm
    return V, Hraw


@dataclass
class Cycle:
    """One restart cycle as the figures read it (a reference run or a device capture)."""
    V: np.ndarray              # [>= final_cols, n]
    cols: int                  # columns committed to H
    final_cols: int            # leading rows of V that are final
    x_in: np.ndarray
    x_out: np.ndarray
    H: np.ndarray              # rotated, [>= cols, >= cols + 1]
    S: np.ndarray
    giv: np.ndarray            # [>= cols, 2]
    presid: float
    Hraw: np.ndarray | None = None     # [>= cols, >= cols + 1]; None: rebuilt from H and giv
    early: dict = field(default_factory=dict)   # {column: nu} committed from the tentative column


def run_cycle(op: Operator, b, x_in, k, scheme) -> Cycle:
    """One GMRES cycle of k columns in op.dtype (SciPy's sequence: v0 = M^-1 r / beta, Arnoldi,
    dlartg rotations, back substitution, x update)."""
    dt = op.dtype
    x_in = np.asarray(x_in).astype(dt)
    r0 = op.presidual(b, x_in)
    beta = np.sqrt(r0 @ r0)
    V, Hraw = arnoldi(op, r0 / beta, k, scheme)
    H, giv, S = givens_qr(Hraw, beta, k)
    y = hess_solve(H, S, k)
    x_out = x_in + y @ V[:k]
    return Cycle(V=V, cols=k, final_cols=k + 1, x_in=x_in, x_out=x_out, H=H, S=S, giv=giv,
                 presid=abs(S[k]), Hraw=None if scheme == "mgs" else Hraw)


def minimiser(op: Operator, b, x_in, k):
    """The longdouble minimiser's correction delta of ||M^-1 (b - A x)|| over x_in + K_k."""
    assert op.dtype is LD
    c = run_cycle(op, b, x_in, k, "cgs2x")
    return c.x_out - c.x_in


# ---------------------------------------------------------------------------------------
# the figures, all in longdouble
# ---------------------------------------------------------------------------------------
def _nrm(v):
    return np.sqrt(v @ v)


def figures(op: Operator, b, cyc: Cycle, delta=None) -> dict:
    """F1 (per column), F2, F3 (vector, beta), F4 (per column: H, giv, S), F5, F6 of a cycle, against
    the longdouble operator ``op``.  delta: the longdouble minimiser's correction for cyc.cols
    columns from cyc.x_in (computed when None)."""
    assert op.dtype is LD
    k, fc = cyc.cols, cyc.final_cols
    V = np.asarray(cyc.V[:fc]).astype(LD)
    giv = np.asarray(cyc.giv)
    out = {}
    # F1: the Arnoldi relation, column by column
    f1 = []
    for c in range(max(fc - 1, 0)):
        if c >= k:
            break
        h = (np.asarray(cyc.Hraw[c, :c + 2]).astype(LD) if cyc.Hraw is not None
             else unrotate_column(cyc.H[c], giv, c))
        Bv = op.B(V[c])
        f1.append(float(_nrm(Bv - h @ V[:c + 2]) / _nrm(Bv)))
    out["F1"] = f1
    # F2: orthonormality of the final columns
    out["F2"] = float(np.max(np.abs(V @ V.T - np.eye(fc, dtype=LD))))
    # F3: the cycle's start
    r0 = op.presidual(b, cyc.x_in)
    beta = _nrm(r0)
    S0 = unrotate_S(cyc.S, giv, k)[0]
    out["F3v"] = float(_nrm(V[0] - r0 / beta))
    out["F3b"] = float(abs(S0 - beta) / beta)
    # F4: the rotated H, the rotations and S against a longdouble Givens QR of the raw columns
    if cyc.Hraw is not None:
        raw = np.zeros((k, k + 2), LD)
        for c in range(k):
            raw[c, :c + 2] = np.asarray(cyc.Hraw[c, :c + 2]).astype(LD)
            if c in cyc.early:
                raw[c, c + 1] = LD(cyc.early[c])
        Hq, gq, Sq = givens_qr(raw, S0, k)
        f4 = []
        for c in range(k):
            hn = _nrm(raw[c, :c + 2])
            f4.append(max(float(_nrm(Hq[c, :c + 2] - np.asarray(cyc.H[c, :c + 2]).astype(LD)) / hn),
                          float(_nrm(gq[c] - giv[c].astype(LD))),
                          float(abs(Sq[c + 1] - LD(cyc.S[c + 1])) / S0)))
        out["F4"] = f4
    # F5: the correction against the longdouble minimiser's
    if delta is None:
        delta = minimiser(op, b, cyc.x_in, k)
    dx = np.asarray(cyc.x_out).astype(LD) - np.asarray(cyc.x_in).astype(LD)
    out["F5"] = float(_nrm(dx - delta) / _nrm(delta))
    # F6: the reported preconditioned residual against the true one
    pr = _nrm(op.presidual(b, cyc.x_out))
    out["F6"] = float(abs(LD(cyc.presid) - pr) / pr)
    return out


def worst(f: dict) -> dict:
    """Each figure as one number (the worst column)."""
    return {k: (max(v) if isinstance(v, list) and v else (0.0 if isinstance(v, list) else v)) for k, v in f.items()}
