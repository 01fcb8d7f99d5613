#!/usr/bin/env python3
"""CPU table of the Neumann-series wrapper: SciPy GMRES iteration counts
with N_k = the degree-(k-1) Neumann series of M^-1 A around each base preconditioner M,

    z_1 = M^-1 r ;  z_{i+1} = z_i + M^-1 (r - A z_i),  i = 1 .. k-1

for k = 1..4.  Bases: BJ(8), line_jacobi seg 25, line_cyclic (x-lines) and, on the 4D operators,
line_product (x . y, seg 25 each, the C4 choice of tools/bench_line_product.py).  rtol 1e-8,
restart 20, twin.rhs, at most 100 restart cycles.  No GPU: everything here is SciPy on the host; the
figures decide which GPU comparisons are worth quoting, nothing else.

    python tools/neumann_cpu_table.py [--out profiles/neumann_cpu_table.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import twin  # noqa: E402

OPERATORS = {
    "S2 (64,32)": twin.Vlasov(2, (64, 32)),
    "(250,160)": twin.Vlasov(2, (250, 160)),
    "S4 (6,5,8,8)": twin.Vlasov(4, (6, 5, 8, 8)),
    "(50,25,6,5) fp32": twin.Vlasov(4, (50, 25, 6, 5), fp32=True),
    "(200,125,3,3) fp32": twin.Vlasov(4, (200, 125, 3, 3), fp32=True),
}
DEGREES = (1, 2, 3, 4)
MAX_CYCLES = 100   # restart cycles: info 100 = not converged within 2000 inner iterations


def cyclic_matrix(ip, ix, d, n, stride, period):
    """A's diagonal plus the couplings between line neighbours modulo period."""
    import scipy.sparse as sp
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(ip, np.int64)))
    cols = np.asarray(ix, np.int64)
    same = (rows % stride == cols % stride) & (rows // (stride * period) == cols // (stride * period))
    di = ((cols // stride) % period - (rows // stride) % period) % period
    keep = (rows == cols) | (same & ((di == 1) | (di == period - 1)))
    return sp.csr_matrix((np.asarray(d, np.float64)[keep], (rows[keep], cols[keep])), shape=(n, n))


def bases(p, ip, ix, d):
    """name -> matvec of M^-1 for the bases that exist on this operator."""
    from scipy.sparse.linalg import splu
    n = p.n
    d64 = np.asarray(d, np.float64)
    out = {}
    Binv = twin.bj_inverse_numpy(ip, ix, d64, n, 8)
    out["BJ(8)"] = lambda r: twin.bj_apply_numpy(Binv, r, n)
    if p.dim == 2:
        sx, px = p.shape[1], p.shape[0]
    else:
        sx, px = p.shape[1] * p.shape[2] * p.shape[3], p.shape[0]
    lj = twin.line_operator(ip, ix, d64, n, sx, 25)
    out["line_jacobi seg 25"] = lj.matvec
    luc = splu(cyclic_matrix(ip, ix, d64, n, sx, px).tocsc(), permc_spec="NATURAL")
    out["line_cyclic"] = luc.solve
    if p.dim == 4:
        sy = p.shape[2] * p.shape[3]
        lu1 = splu(twin.line_matrix(ip, ix, d64, n, sx, 25).tocsc(), permc_spec="NATURAL")
        lu2 = splu(twin.line_matrix(ip, ix, d64, n, sy, 25).tocsc(), permc_spec="NATURAL")
        D = twin.scipy_csr(ip, ix, d64, n).diagonal()
        out["line_product"] = lambda r: lu2.solve(D * lu1.solve(r))
    return out


def neumann(A, M, degree):
    def mv(r):
        r = np.asarray(r, np.float64).reshape(-1)
        z = M(r)
        for _ in range(degree - 1):
            z = z + M(r - A @ z)
        return z
    return mv


def main():
    from scipy.sparse.linalg import LinearOperator
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neumann_cpu_table.json"))
    args = ap.parse_args()
    rows = []
    for oname, p in OPERATORS.items():
        ip, ix, d = twin.generate(p)
        A = twin.scipy_csr(ip, ix, np.asarray(d, np.float64), p.n)
        b = twin.rhs(p.n)
        for bname, M in bases(p, ip, ix, d).items():
            for k in DEGREES:
                op = LinearOperator((p.n, p.n), matvec=neumann(A, M, k), dtype=np.float64)
                s = twin.scipy_gmres(A, b, op, rtol=1e-8, restart=20, maxiter=MAX_CYCLES)
                rec = {"operator": oname, "n": p.n, "base": bname, "degree": k, "inner": s.inner_iters,
                       "info": s.info, "resid_rel": s.true_resid / s.b_norm}
                rows.append(rec)
                print(json.dumps(rec), flush=True)
    with open(args.out, "w") as f:
        json.dump({"rtol": 1e-8, "restart": 20, "maxiter": MAX_CYCLES, "rhs": "twin.rhs", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
