"""Deterministic test matrices that take the branches the Vlasov operators never do -- TEST
INFRASTRUCTURE ONLY (numpy / scipy; imported by ``tests/`` alone).

Every matrix the rest of the suite uses is a Vlasov operator or the diagonally dominant
``ragged`` fixture, so partial pivoting, the tridiagonal-factor check's accuracy reasons, the
Arnoldi columns past 24 and the breakdown paths of the scalar step never run there.  The builders
below make inputs that do, each returned as ``(indptr int32, indices int32, data)`` like
``twin.generate``.
"""
from __future__ import annotations

import numpy as np

# ---------------------------------------------------------------------------------------
# block Jacobi: blocks that need a row swap in every column
# ---------------------------------------------------------------------------------------


def pivot_n(bs: int) -> int:
    """Rows of the pivot_blocks matrix: five whole blocks and a padded one (bs 1: 7 rows)."""
    return 7 if bs == 1 else 5 * bs + bs // 2


def _pivot_dense(bs: int, seed: int, ints: bool, fp32: bool):
    """Per block: (stored dense block, effective dense block).  Block 1's row ``dup_row`` stores
    ``dup_val`` a second time at ``dup_col``; the effective block is what toarray() would give."""
    rng = np.random.default_rng([seed, bs, int(ints)])
    n = pivot_n(bs)
    out = []
    for b0 in range(0, n, bs):
        m = min(bs, n - b0)
        while True:
            if ints:
                blk = rng.integers(-3, 4, size=(m, m)).astype(np.float64)
            else:
                blk = rng.standard_normal((m, m))
            if m > 1:
                np.fill_diagonal(blk, 0.0)      # every column needs a row swap
            elif ints and blk[0, 0] == 0.0:
                continue                        # a 1 x 1 block cannot have a zero diagonal
            if fp32:
                blk = blk.astype(np.float32).astype(np.float64)
            eff = blk.copy()
            dup = None
            if b0 == bs:                        # block 1 carries the non-canonical row
                i = min(1, m - 1)
                cand = [c for c in range(m) if blk[i, c] != 0.0]
                if not cand:
                    continue
                dup = (i, cand[0], 1.0)
                eff[i, cand[0]] += 1.0
            if np.linalg.matrix_rank(eff) == m and np.linalg.cond(eff) < 1e4:
                out.append((blk, eff, dup))
                break
    return out


def pivot_blocks(bs: int, seed: int = 0, ints: bool = False, fp32: bool = False):
    """CSR of n = 5 bs + bs // 2 rows (bs 1: 7) whose dense bs x bs diagonal blocks have ZERO
    diagonals, so Gauss-Jordan swaps a row in every column; the short last block is padded by the
    setup.  Entries: standard_normal, or integers in [-3, 3] (``ints``: many exact |a| ties, which
    the rule "first row of largest |a|" must break the same way everywhere).  Blocks are resampled
    until rank is full and cond < 1e4.  (Blocks of one row -- bs 1, and the tail of bs 2 and 3 --
    keep a nonzero entry.)

    Also: two off-block entries, (0, n-1) and (n-1, 0), which the setup must ignore; and row
    bs + 1 (bs 1: row 1) stored non-canonically -- an off-block entry first, the block entries in
    descending column order, one of them twice (the second time with value 1): duplicates add up,
    as csr_matrix.toarray() does, and SpMV sums in stored order.

    ``fp32``: the data as float32 (drives the VT = float kernels; the oracle takes the same array).
    """
    n = pivot_n(bs)
    indptr, indices, data = [0], [], []
    blocks = _pivot_dense(bs, seed, ints, fp32)
    for r in range(n):
        b0 = (r // bs) * bs
        blk, _, dup = blocks[r // bs]
        i = r - b0
        cols = [b0 + c for c in range(blk.shape[1]) if blk[i, c] != 0.0]
        vals = [blk[i, c - b0] for c in cols]
        if r == 0:
            cols.append(n - 1)
            vals.append(3.0)
        if r == n - 1:
            cols.insert(0, 0)
            vals.insert(0, -2.0)
        if dup is not None and i == dup[0]:
            cols, vals = cols[::-1], vals[::-1]
            k = cols.index(b0 + dup[1])
            cols.insert(k + 1, b0 + dup[1])
            vals.insert(k + 1, dup[2])
            cols.insert(0, n - 2)               # an off-block entry first: columns unsorted
            vals.insert(0, 0.5)
        indices += cols
        data += vals
        indptr.append(len(indices))
    return (np.asarray(indptr, np.int32), np.asarray(indices, np.int32),
            np.asarray(data, np.float32 if fp32 else np.float64))


def singular_blocks(bs: int, kind: str, block: int = 2, seed: int = 0):
    """pivot_blocks(bs, seed) with diagonal block ``block`` made singular by an EXACT zero pivot:
    ``kind="col"`` drops the block's first column, ``kind="row"`` its first row (off-block entries
    stay).  ``block=-1``: the padded last block.  (Not duplicated rows: d * (a / d) != a in
    floating point, so that pivot is tiny but not zero.)"""
    if kind not in ("col", "row"):
        raise ValueError("kind must be 'col' or 'row'")
    ip, ix, d = pivot_blocks(bs, seed)
    n = ip.shape[0] - 1
    nb = (n + bs - 1) // bs
    b0 = (block % nb) * bs
    b1 = min(n, b0 + bs)
    rows = np.repeat(np.arange(n), np.diff(ip))
    inblk = (rows >= b0) & (rows < b1) & (ix >= b0) & (ix < b1)
    drop = inblk & ((ix == b0) if kind == "col" else (rows == b0))
    keep = ~drop
    cnt = np.bincount(rows[keep], minlength=n)
    ip2 = np.zeros(n + 1, np.int32)
    np.cumsum(cnt, out=ip2[1:])
    return ip2, ix[keep].copy(), d[keep].copy()


# ---------------------------------------------------------------------------------------
# block Jacobi: tridiagonal blocks on which Thomas without pivoting is (in)accurate
# ---------------------------------------------------------------------------------------

TRI_NB = 6
# Default seeds, chosen on the host (scan of seeds 0 .. 2999, first hits) so that at once
#   * d0 = 1e-8 is > 50x over and d0 = 1e-4 > 50x under the setup check's bound,
#   * every block has cond <= 40,
#   * at d0 = 1e-4 the tridiagonal apply (tri_scan_apply below) of twin.rhs(n) lies within HALF of
#     the suite's tridiagonal-apply bar (rtol 1e-12, atol 1e-14 max|z|) of the inverse apply.
# The last condition is what makes seeds rare: at d0 = 1e-4 the factors carry an error of
# ~1e-12 of the largest inverse entry (growth 1/d0 x eps), the size of that bar itself; a
# typical seed lands at 0.7 .. 1.5 x the bar.  What the setup check guarantees for an accepted
# block is its own bound, 1e-10.
TRI_SEED = {2: 80, 4: 1477, 8: 2106}


def tri_blocks(bs: int, d0: float, seed: int | None = None):
    """Six tridiagonal bs x bs diagonal blocks (bs 2, 4, 8; n = 6 bs): sub- and super-diagonal
    1 + U(0,1), diagonal 2 + U(0,1), the FIRST diagonal entry of each block ``d0``; weak
    nonsymmetric coupling between neighbouring blocks (1e-2 above, -5e-3 below the block diagonal,
    periodic), which the setup ignores.

    The leading pivot of Thomas without pivoting is d0, so its factors lose accuracy as d0
    shrinks while the block stays well conditioned (cond <= 36 at the default seeds TRI_SEED).
    Measured with the setup kernel's check (max |factor solve - Gauss-Jordan inverse| against
    1e-10 x the largest inverse entry; tests/test_oracle_cases.py restates and asserts it), worst
    block of the six, bs 2 / 4 / 8:
        d0 = 1e-8 : 3.9e-8 / 2.9e-8 / 3.4e-8    -> > 290x over the bound: must be rejected
        d0 = 1e-4 : 1.7e-12 / 1.7e-12 / 1.4e-12 -> > 58x under it: must stay accepted
        d0 = 1e-6 : ~1e-10, borderline, not used.
    ``d0 = 0.0`` (use bs = 2): the first row's super-diagonal is set to 1; the blocks are
    nonsingular with a zero leading pivot (the tiny-pivot reason)."""
    if bs not in (2, 4, 8):
        raise ValueError("bs must be 2, 4 or 8")
    rng = np.random.default_rng([TRI_SEED[bs] if seed is None else seed, bs, 77])
    n = TRI_NB * bs
    indptr, indices, data = [0], [], []
    for r in range(n):
        i = r % bs
        sub, dia, sup = 1.0 + rng.random(), 2.0 + rng.random(), 1.0 + rng.random()
        if i == 0:
            dia = d0
            if d0 == 0.0:
                sup = 1.0
        ent = {}
        if i > 0:
            ent[r - 1] = sub
        ent[r] = dia
        if i < bs - 1:
            ent[r + 1] = sup
        ent[(r + bs) % n] = ent.get((r + bs) % n, 0.0) + 1e-2
        ent[(r - bs) % n] = ent.get((r - bs) % n, 0.0) - 5e-3
        for c in sorted(ent):
            indices.append(c)
            data.append(ent[c])
        indptr.append(len(indices))
    return np.asarray(indptr, np.int32), np.asarray(indices, np.int32), np.asarray(data, np.float64)


def thomas_factors(blk: np.ndarray):
    """Thomas without pivoting on the tridiagonal block ``blk`` as the device setup runs it:
    u_0 = d_0, l_i = sub_i / u_{i-1}, u_i = d_i - l_i sup_{i-1}, m_i = 1 / u_i, g_i = sup_i m_i.
    Returns (l, m, g, tiny) with tiny: some |u_i| <= 1e-12 (|sub_i| + |d_i| + |sup_i|)."""
    bs = blk.shape[0]
    sub = np.array([blk[i, i - 1] if i > 0 else 0.0 for i in range(bs)])
    dia = np.diag(blk).copy()
    sup = np.array([blk[i, i + 1] if i + 1 < bs else 0.0 for i in range(bs)])
    l, m, g = np.zeros(bs), np.zeros(bs), np.zeros(bs)
    tiny = False
    u = dia[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(bs):
            if i > 0:
                l[i] = sub[i] / u
                u = dia[i] - l[i] * sup[i - 1]
            if not abs(u) > 1e-12 * (abs(sub[i]) + abs(dia[i]) + abs(sup[i])):
                tiny = True
            m[i] = 1.0 / u
            g[i] = sup[i] * m[i]
    return l, m, g, tiny


def thomas_check(blk: np.ndarray, inv: np.ndarray):
    """The tridiagonal-factor check of the device setup restated; returns (tiny_pivot, err, mag)
    with err the largest |factor solve of e_k - inv[:, k]| and mag the largest |inv| entry.  The
    setup rejects the block when tiny_pivot or err > 1e-10 mag."""
    bs = blk.shape[0]
    l, m, g, tiny = thomas_factors(blk)
    err = 0.0
    with np.errstate(invalid="ignore"):
        for k in range(bs):
            d = np.zeros(bs)
            for i in range(bs):
                d[i] = (1.0 if i == k else 0.0) - (l[i] * d[i - 1] if i > 0 else 0.0)
            zn = 0.0
            for i in range(bs - 1, -1, -1):
                zn = m[i] * d[i] - (g[i] * zn if i + 1 < bs else 0.0)
                e = abs(zn - inv[i, k])
                err = e if e > err else err      # fmax: a NaN difference is skipped, as on the device
    return tiny, float(err), float(np.abs(inv).max())


def tri_scan_apply(l, m, g, y):
    """The device's tridiagonal block apply restated: d_i = y_i - l_i d_{i-1} and
    z_i = m_i d_i - g_i z_{i+1} as two affine scans of log2(bs) steps over the block's rows."""
    bs = y.shape[0]
    idx = np.arange(bs)
    A, B = np.array(y, np.float64), -np.asarray(l, np.float64)
    off = 1
    while off < bs:
        Ap, Bp = np.r_[np.zeros(off), A[:-off]], np.r_[np.zeros(off), B[:-off]]
        A, B = np.where(idx >= off, A + B * Ap, A), np.where(idx >= off, B * Bp, B)
        off <<= 1
    A, B = m * A, -np.asarray(g, np.float64)
    off = 1
    while off < bs:
        An, Bn = np.r_[A[off:], np.zeros(off)], np.r_[B[off:], np.zeros(off)]
        A, B = np.where(idx + off < bs, A + B * An, A), np.where(idx + off < bs, B * Bn, B)
        off <<= 1
    return A


# ---------------------------------------------------------------------------------------
# GMRES: operators whose convergence depends on the high Arnoldi columns
# ---------------------------------------------------------------------------------------


def outlier_op(n: int = 1025, nout: int = 26, lo: float = 1e-7, spread: float = 0.05,
               off: float = 0.02, seed: int = 11, signs: bool = True):
    """Tridiagonal operator: diagonal 1 + spread U(0,1) with ``nout`` outliers at
    linspace(3, n-4, nout) set to geomspace(lo, 0.5, nout) (every third negated with ``signs``),
    constant super-diagonal ``off`` and sub-diagonal -off/2.  n odd: the i + 1 < n tails of the
    row-pair kernels run.

    GMRES has to resolve one outlier eigenvalue after the other, so a restart cycle only pays off
    when its high columns are right.  With b = twin.rhs(n), rtol 1e-10, maxiter 40:

    R = outlier_op()  (cond ~ 4.8e3), oracle/vtk_oracle.c (SciPy's gmres agrees: see
    tests/test_oracle_cases.py):
        restart 20 : info 40, 800 inner iterations, error vs dense solve 4.3e-2 (not converged)
        restart 31 : info 0, 243, 1.07e-9
        restart 32 : info 0, 253, 9.7e-10
        restart 40 : info 0, 123, 8.9e-10
      (restart 24 / 25: 689 iterations / not converged -- the count jumps there, no bars.)

    Q = outlier_op(1025, 16, 1e-8, 1e-3, 1e-3, seed=12, signs=False)  (cond ~ 1e6): iteration
    counts depend on the Gram-Schmidt variant (oracle 87, numpy MGS 84, CGS2 92, CGS 99 at restart
    32), so Q only gets weak bars."""
    rng = np.random.default_rng(seed)
    dia = 1.0 + spread * rng.random(n)
    pos = np.linspace(3, n - 4, nout).astype(np.int64)
    val = np.geomspace(lo, 0.5, nout)
    if signs:
        val[::3] *= -1.0
    dia[pos] = val
    indptr, indices, data = [0], [], []
    for r in range(n):
        if r > 0:
            indices.append(r - 1)
            data.append(-off / 2)
        indices.append(r)
        data.append(dia[r])
        if r + 1 < n:
            indices.append(r + 1)
            data.append(off)
        indptr.append(len(indices))
    return np.asarray(indptr, np.int32), np.asarray(indices, np.int32), np.asarray(data, np.float64)


def op_R():
    return outlier_op()


def op_Q():
    return outlier_op(1025, 16, 1e-8, 1e-3, 1e-3, seed=12, signs=False)


LOW_DEGREE_VALUES = (1.0, 2.5, -3.0, 7.0, 0.5)


def low_degree_diag(k: int, n: int = 1025):
    """Diagonal operator with the k distinct values LOW_DEGREE_VALUES[:k] repeating: the Krylov
    space of any b has dimension k, so GMRES converges in exactly k steps and step k + 1 (if
    taken) meets an exhausted space -- h_{k+1,k} = 0 up to rounding (the breakdown branch)."""
    if not 1 <= k <= len(LOW_DEGREE_VALUES):
        raise ValueError("k out of range")
    d = np.asarray(LOW_DEGREE_VALUES[:k])[np.arange(n) % k]
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d.astype(np.float64)


def dense(indptr, indices, data):
    """toarray() of the CSR (duplicates add)."""
    n = indptr.shape[0] - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(A, (rows, indices), np.asarray(data, np.float64))
    return A
