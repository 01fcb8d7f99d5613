"""BiCGStab across ranks without a GPU: the premise of the bars the multi-rank GPU tests use.

Across ranks every dot of the iteration is a sum over the ranks' slabs (an all-reduce of per-rank
sums) instead of one sum over the whole vector.  The NumPy twin of scipy.sparse.linalg.bicgstab
(tests/test_bicgstab_host.py) is run here with such rank-partitioned dots -- the sum, in rank order,
of np.dot of each slab, slabs on whole x lines (2D) or x planes (4D) -- and must stay inside the
project's BiCGStab bars against the np.dot twin: info equal, |iterations - ref| <= max(2, ceil(0.15
ref)), ||x - x_ref|| <= 4 rtol ||x_ref||.  Two line-preconditioned cases are sharp (the partition
keeps the count and the exit and moves x by <= 2e-16 relative); their counts and exits are pinned
here and the GPU tests hold them to equality.

The line preconditioner's segments start at each rank's first line, so M is the same at every rank
count only when the segment divides each rank's lines (planes): LINE_SEG below.
"""
import functools
import math

import numpy as np
import pytest

from oracle import coracle, twin
from test_bicgstab_host import bicgstab_twin

MAXIT = 500
# segment of the line preconditioner that divides every rank's lines / planes: (case, world) -> seg
LINE_SEG = {("S2", 2): 8, ("S2", 4): 8, ("S4", 2): 3, ("S4", 3): 2, ("S4F", 2): 3, ("S4F", 3): 2, ("C1", 2): 25}


def slab_unit(p):
    """Rows of one x line (2D) or one x plane (4D): the ranks' slabs are whole multiples of it."""
    return p.shape[1] if p.dim == 2 else p.shape[1] * p.shape[2] * p.shape[3]


def slab_offsets(name, world):
    p = twin.CONFIGS[name]
    unit = slab_unit(p)
    units = p.n // unit
    assert units * unit == p.n and units % world == 0, (name, world)
    return np.arange(world + 1, dtype=np.int64) * (units // world) * unit


def dot_slabs(offs):
    """The dot across ranks: each rank's np.dot of its slab, summed in rank order."""
    def dot(a, c):
        s = 0.0
        for r in range(len(offs) - 1):
            s += float(np.dot(a[offs[r]:offs[r + 1]], c[offs[r]:offs[r + 1]]))
        return s
    return dot


@functools.lru_cache(maxsize=None)
def host_system(name):
    p = twin.CONFIGS[name]
    ip, ix, d = coracle.generate(p)
    for a in (ip, ix, d):
        a.setflags(write=False)
    return p, (ip, ix, d), twin.scipy_csr(ip, ix, d.astype(np.float64), p.n), twin.rhs(p.n)


@functools.lru_cache(maxsize=None)
def host_prec(name, kind, seg=0):
    """The twin's M as a callable: None, the oracle's BJ inverse rows (kind bjN) or its line factors
    with segment seg."""
    p, csr, A, b = host_system(name)
    if kind == "none":
        return None
    if kind.startswith("bj"):
        inv = coracle.bj_setup(*csr, int(kind[2:]))
        return lambda r: coracle.bj_apply(inv, np.ascontiguousarray(r))
    lf = coracle.line_setup(*csr, slab_unit(p), seg)
    return lambda r: coracle.line_apply(lf, np.ascontiguousarray(r))


@functools.lru_cache(maxsize=None)
def ref(name, kind, rtol, seg=0, maxiter=MAXIT, world=0, x0_seed=None, b_zero_to=0):
    """(x, info, iterations, half_step) of the twin: np.dot (world 0) or the dots of `world` slabs.
    b_zero_to > 0: b zero on rows [0, b_zero_to)."""
    p, csr, A, b = host_system(name)
    if b_zero_to:
        b = b.copy()
        b[:b_zero_to] = 0.0
    x0 = None
    if x0_seed is not None:   # non-zero on the last slab of two only
        x0 = np.zeros(p.n)
        x0[p.n // 2:] = twin.rhs(p.n, seed=x0_seed)[p.n // 2:]
    dot = dot_slabs(slab_offsets(name, world)) if world else np.dot
    out = bicgstab_twin(A, b, x0, rtol=rtol, maxiter=maxiter, M=host_prec(name, kind, seg), dot=dot)
    out[0].setflags(write=False)
    return out


CASES = [("S2", 2), ("S2", 4), ("S4", 2), ("S4", 3), ("S4F", 2), ("S4F", 3)]


@pytest.mark.parametrize("rtol", [1e-5, 1e-8])
@pytest.mark.parametrize("kind", ["none", "bj8", "line"])
@pytest.mark.parametrize("name,world", CASES)
def test_partitioned_dots_stay_inside_the_bars(name, world, kind, rtol):
    seg = LINE_SEG[(name, world)] if kind == "line" else 0
    x0, info0, its0, half0 = ref(name, kind, rtol, seg)
    x, info, its, half = ref(name, kind, rtol, seg, world=world)
    rel = np.linalg.norm(x - x0) / np.linalg.norm(x0)
    print(f"iterations {its} (np.dot {its0}) half {half} ({half0}) x difference / rtol {rel / rtol:.3f}")
    assert info == info0 == 0
    assert abs(its - its0) <= max(2, math.ceil(0.15 * its0)), (its, its0)
    assert rel <= 4 * rtol, rel


# the sharp cases: (case, world, rtol) -> (iterations, half_step) of the twin, whatever its dots
SHARP = {("S2", 2, 1e-5): (6, 1), ("S2", 4, 1e-5): (6, 1), ("S2", 2, 1e-8): (9, 0), ("S2", 4, 1e-8): (9, 0),
         ("C1", 2, 1e-5): (5, 0), ("C1", 2, 1e-8): (8, 0)}


@pytest.mark.parametrize("name,world,rtol", sorted(SHARP))
def test_sharp_line_cases(name, world, rtol):
    """S2 / line seg 8 and C1 / line seg 25: the partition keeps the count and the exit (both exits
    occur: the half step at S2 1e-5, the top elsewhere) and moves x by a few ulp (printed)."""
    seg = LINE_SEG[(name, world)]
    x0, info0, its0, half0 = ref(name, "line", rtol, seg)
    x, info, its, half = ref(name, "line", rtol, seg, world=world)
    rel = np.linalg.norm(x - x0) / np.linalg.norm(x0)
    print(f"iterations {its} half {half} x difference {rel:.3e}")
    assert info == info0 == 0
    assert (its0, half0) == SHARP[(name, world, rtol)] == (its, half)
    assert rel <= 1e-9, rel   # the project's bar for sharp cases, as the GPU tests hold them
