"""BiCGStab's first iterations pinned to the extended-precision reference (oracle/bicgstab.py).

The solve-level bars of tests/test_gpu_bicgstab.py (x to 4 rtol, the count to 15 %) are loose
because BiCGStab amplifies summation-order noise over a long run; a kernel that is wrong at the
1e-10 level passes them.  The kernels are the same code at every iteration (first / not first, the
four scalar phases, the half-step exit), and after one, two and three iterations nothing has been
amplified yet.  So ``vk.bicgstab(A, b, x0, rtol=0, atol=0, maxiter=k, M=M)`` for k = 1, 2, 3 is held
to the longdouble run of SciPy's loop on B's own data (A from the CSR values, M^-1 from A's blocks /
line matrices in longdouble, never the device's factors):

* info == k, iterations == k, half_step == 0;
* ||x_dev - x_k^LD|| / ||x_k^LD|| <= 16 R_k, R_k the same figure of the plain float64 NumPy loop
  (the worst of three summation orders of its dots, floored at 2^-53), computed here;
  tests/test_bicgstab_reference.py holds 16 R_k <= 1e-12 for every case of this module and shows
  which planted defects that bar sees;
* |stats.rnorm - ||b - A x_dev||_LD| <= 16 2^-53 (||b|| + ||A||_inf ||x_dev||): the field is the
  true residual of the returned x.

The half-step cases pass an atol inside 2 ||s_k|| <= atol <= ||r_{k-1}|| / 2 of the longdouble run
and rtol = 0 (no summation order can move the exit): info == 0, half_step == 1, iterations == k
and the same bar on x.  Cases and references are tests/test_bicgstab_reference.py's.
"""
import numpy as np
import pytest

from oracle import bicgstab as bc
from test_bicgstab_host import general_csr
from test_bicgstab_reference import (GRID_OPS, HALF, KMAX, MARGIN, RANKS, U, cyclic_geometry, half_reference,
                                     line_geometry, ops, params_of, product_geometry, reference, system, x0_of)

pytestmark = pytest.mark.gpu

LD = bc.LD
LAYOUTS = ("csr", "sell")


# ---- host side --------------------------------------------------------------------------------
def _nrm(v):
    return np.sqrt(v @ v)


def norm_inf(name):
    ip, _, d = system(name)[0]
    return float(np.add.reduceat(np.abs(np.asarray(d, np.float64)), np.asarray(ip[:-1], np.int64)).max())


def check_iterate(tag, name, prec, x, st, x_ld, R_k, bad):
    """The figure of x against the longdouble iterate and the reported residual against the true
    one; prints both, appends what is over its bar to ``bad``."""
    _, _, b = system(name)
    fig = bc.figure(x, x_ld)
    xl = np.asarray(x).astype(LD)
    res = b.astype(LD) - ops(name, prec).ld.A(xl)
    rn = _nrm(res)
    rbar = MARGIN * U * (float(_nrm(b)) + norm_inf(name) * float(_nrm(xl)))
    rerr = float(abs(LD(st.rnorm) - rn))
    print(f"BCG|{tag}|dev {fig:.3e}|ref {R_k:.3e}|x{fig / R_k:.2f}|rnorm err {rerr:.3e}|bar {rbar:.3e}")
    if not fig <= MARGIN * R_k:
        bad.append((tag, "x", fig, R_k, fig / R_k))
    if not rerr <= rbar:
        bad.append((tag, "rnorm", rerr, rbar))


def run_steps(tag, vk, A, M, name, prec, x0, bad):
    """k = 1, 2, 3 truncated runs of one (operator, preconditioner, x0)."""
    _, _, b = system(name)
    ld, R = reference(name, prec, x0)
    for k in range(1, KMAX + 1):
        x, info = vk.bicgstab(A, b, x0_of(name, x0), rtol=0.0, atol=0.0, maxiter=k, M=M)
        st = vk.last_bicgstab_stats()
        assert (info, st.iterations, st.half_step) == (k, k, 0), (tag, k, info, st.iterations, st.half_step)
        assert st.atol_eff == 0.0
        check_iterate(f"{tag} x0={x0} k={k}", name, prec, x, st, ld.xs[k - 1], R[k - 1], bad)


# ---- device side ------------------------------------------------------------------------------
def vparams(vk, p):
    return vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)


@pytest.fixture(scope="module")
def dev_ops(vk_lib, gpu):
    """The operators, assembled on the device; the references read the same CSR bits."""
    out = {}

    def get(name):
        if name not in out:
            if name == "G":
                A = vk_lib.csr_matrix(general_csr(), ctx=gpu)
            else:
                A = vk_lib.vlasov_operator(vparams(vk_lib, params_of(name)), ctx=gpu)
            for dev, host in zip(A.download(), system(name)[0]):
                assert np.array_equal(dev, host), f"{name}: the device operator is not the reference's"
            out[name] = A
        return out[name]
    yield get
    for A in out.values():
        A.close()


# variant -> (reference preconditioner, block size, mode, bcg_fuse); the fused forms (phat = M p, shat
# = M s inside k_bcg_p / k_bcg_s) exist for bs 1, 2, 4, 8; BJ(16) takes the separate apply
BJ_VARIANTS = {f"bj{bs}{'-' + mode if mode != 'auto' else ''}-fuse{fuse}": (f"bj{bs}", bs, mode, fuse)
               for bs, mode in ((8, "tridiag"), (8, "inverse"), (4, "auto"), (2, "auto"), (1, "auto")) for fuse in (1, 0)}
BJ_VARIANTS["bj16"] = ("bj16", 16, "auto", None)
GRID_VARIANTS = ["none"] + list(BJ_VARIANTS) + ["line"]


def make_prec(vk, A, name, variant):
    """(M, everything to close in order, the reference preconditioner, bcg_fuse or None)."""
    p = None if name == "G" else params_of(name)
    if variant == "none":
        return None, [], "none", None
    if variant in BJ_VARIANTS:
        prec, bs, mode, fuse = BJ_VARIANTS[variant]
        M = vk.block_jacobi(A, bs, mode)
        if mode != "auto":
            assert M.mode == mode
        return M, [M], prec, fuse
    if variant == "line":
        M = vk.line_jacobi(A, *line_geometry(p))
        return M, [M], "line", None
    if variant == "product":
        M = vk.line_product(A, *product_geometry(p))
        return M, [M], "product", None
    if variant in ("cyclic", "cyclic-span"):
        stride, period, seg = cyclic_geometry(p)
        M = vk.line_cyclic(A, stride, period, seg, span=variant.endswith("span"))
        return M, [M], "cyclic", None
    if variant == "neumann":
        base = vk.block_jacobi(A, 8)
        M = vk.neumann(A, base, 2)
        return M, [M, base], "neumann", None
    raise KeyError(variant)


def run_variant(vk, gpu, A, name, variant, layouts, bad):
    for layout in layouts:
        if layout:
            A.set_layout(layout)
        try:
            M, owned, prec, fuse = make_prec(vk, A, name, variant)
            try:
                with gpu.tuning(**({} if fuse is None else {"bcg_fuse": fuse})):
                    for x0 in (0, 1):
                        run_steps(f"{name} {variant} {layout or 'auto'}", vk, A, M, name, prec, x0, bad)
            finally:
                for o in owned:
                    o.close()
        finally:
            if layout:
                A.set_layout("auto")


# ---- 1. the grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", GRID_VARIANTS)
@pytest.mark.parametrize("name", GRID_OPS)
def test_first_iterations_grid(vk_lib, gpu, dev_ops, name, variant):
    """S2 (2048 rows), S4 / S4F (1920) and C0 (10 000) in both layouts, from x0 = 0 and x0 != 0."""
    bad = []
    run_variant(vk_lib, gpu, dev_ops(name), name, variant, LAYOUTS, bad)
    assert not bad, bad


# ---- 2. the other preconditioners, a partial workgroup, a general CSR -------------------------
OTHERS = [("S4", "product", (None,)), ("S4", "cyclic", (None,)), ("S2", "cyclic", (None,)), ("S2", "cyclic-span", (None,)),
          ("S2", "neumann", (None,)), ("V7", "bj8-tridiag-fuse1", LAYOUTS), ("V7", "bj8-inverse-fuse1", LAYOUTS),
          ("V7", "none", LAYOUTS), ("G", "none", LAYOUTS), ("G", "bj8-inverse-fuse1", LAYOUTS),
          ("G", "bj8-inverse-fuse0", LAYOUTS)]


@pytest.mark.parametrize("name,variant,layouts", OTHERS, ids=[f"{a}-{b}" for a, b, _ in OTHERS])
def test_first_iterations_others(vk_lib, gpu, dev_ops, name, variant, layouts):
    """The line product and the cyclic y-lines on S4, the cyclic x-lines (plain and spanning) and
    neumann(BJ(8), 2) on S2, V7 = Vlasov(2, (7, 24)) with n = 168, the general CSR of
    tests/test_bicgstab_host.py."""
    bad = []
    run_variant(vk_lib, gpu, dev_ops(name), name, variant, layouts, bad)
    assert not bad, bad


# ---- 3. the half-step exit ----------------------------------------------------------------------
HALF_DEVICE = {("S2", "line", 0): ("line",), ("S2", "line", 1): ("line",), ("S2", "cyclic", 0): ("cyclic", "cyclic-span"),
               ("C0", "bj8", 0): ("bj8-tridiag-fuse1", "bj8-tridiag-fuse0", "bj8-inverse-fuse1")}


def test_half_device_covers_the_cases():
    assert set(HALF_DEVICE) == set(HALF)


@pytest.mark.parametrize("case", sorted(HALF), ids=lambda c: f"{c[0]}-{c[1]}-x0{c[2]}")
def test_half_step_exit(vk_lib, gpu, dev_ops, case):
    name, prec, x0 = case
    k, atol, ld, R = half_reference(*case)
    _, _, b = system(name)
    A = dev_ops(name)
    bad = []
    for variant in HALF_DEVICE[case]:
        M, owned, vprec, fuse = make_prec(vk_lib, A, name, variant)
        assert vprec == prec
        try:
            with gpu.tuning(**({} if fuse is None else {"bcg_fuse": fuse})):
                x, info = vk_lib.bicgstab(A, b, x0_of(name, x0), rtol=0.0, atol=atol, maxiter=10, M=M)
            st = vk_lib.last_bicgstab_stats()
            assert (info, st.iterations, st.half_step) == (0, k, 1), (variant, info, st.iterations, st.half_step, k)
            assert st.atol_eff == atol
            check_iterate(f"half {name} {variant} x0={x0} k={k}", name, prec, x, st, ld.x, R[k - 1], bad)
        finally:
            for o in owned:
                o.close()
    assert not bad, bad


# ---- 4. device tensors ------------------------------------------------------------------------
def test_device_tensors_same_bits(vk_lib, gpu, dev_ops):
    import torch
    name = "S2"
    _, _, b = system(name)
    x0 = x0_of(name, 1)
    A = dev_ops(name)
    M = vk_lib.block_jacobi(A, 8)
    dev = torch.device("cuda", gpu.device)
    try:
        for k in range(1, KMAX + 1):
            x, info = vk_lib.bicgstab(A, b, x0, rtol=0.0, atol=0.0, maxiter=k, M=M)
            st = vk_lib.last_bicgstab_stats()
            tb, tx0 = torch.from_numpy(np.array(b)).to(dev), torch.from_numpy(np.array(x0)).to(dev)
            tx, tinfo = vk_lib.bicgstab(A, tb, tx0, rtol=0.0, atol=0.0, maxiter=k, M=M)
            tst = vk_lib.last_bicgstab_stats()
            assert isinstance(tx, torch.Tensor) and tx.is_cuda
            assert (tinfo, tst.iterations, tst.half_step, tst.rnorm) == (info, st.iterations, st.half_step, st.rnorm)
            assert np.array_equal(tx.cpu().numpy(), x)
            assert np.array_equal(tx0.cpu().numpy(), x0)      # x0 is not written
    finally:
        M.close()


# ---- 5. ranks sharing the GPU (host-staged communicator) ---------------------------------------
@pytest.mark.parametrize("name,world", sorted(RANKS))
def test_first_iterations_across_ranks(name, world):
    """S2 / BJ(8) and S4 / line in x-slabs on two and three ranks through the worker of
    tests/test_gpu_bicgstab_ranks.py: the gathered x under the one-rank bar, info, iterations and
    rnorm the same bits on every rank (k_bcg_reduce and the all-reduced records)."""
    from test_gpu_bicgstab_ranks import _parity_run
    prec = RANKS[(name, world)]
    kind = "bj8" if prec == "bj8" else "line"
    meta, xs, _ = _parity_run(name, world, None, steps=((kind, "auto", tuple(range(1, KMAX + 1))),))
    ld, R = reference(name, prec, 0)
    assert len(meta) == world and len(meta[0]) == KMAX
    bad = []
    for i, m in enumerate(meta[0]):
        k = m["maxiter"]
        assert k == i + 1 and (m["info"], m["iterations"], m["half_step"]) == (k, k, 0), m
        for other in meta[1:]:
            for key in ("info", "iterations", "half_step", "rnorm", "bnorm", "atol_eff"):
                assert other[i][key] == m[key], (key, other[i][key], m[key])
        from types import SimpleNamespace
        st = SimpleNamespace(rnorm=float.fromhex(m["rnorm"]))
        check_iterate(f"ranks {name} {kind} world={world} k={k}", name, prec, xs[i], st, ld.xs[k - 1], R[k - 1], bad)
    assert not bad, bad
