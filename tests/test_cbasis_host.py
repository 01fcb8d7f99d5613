"""Compressed-basis GMRES without a device: the NumPy restatement (tests/cbasis_ref.py) that the GPU
tests of tests/test_gpu_cbasis.py are held to, the ABI additions, and the entry layer.

The restatement is SciPy's control flow around a float64 CGS2 Arnoldi that rounds every stored column
to float32.  What is established here:

* with the float64 basis and SciPy's whole ptol schedule it counts exactly the inner iterations of
  ``scipy.sparse.linalg.gmres`` itself on S2 / BJ(8), S4F / BJ(8) and S2 / x-line (line Jacobi,
  segments of 25 lines) at restart 20 and 5, rtol 1e-8, and restart 20, rtol 1e-12 -- so its control
  flow is SciPy's, and it is what the device runs;
* the iteration table the feature was argued with (``test_issue_table``) is reproduced entry for entry
  with SciPy's ptol test held against the solve's first ptol in every cycle (``schedule="fixed"``):
  68 = 68 in 6 cycles, 69 = 69, 106 = 106; 75 = 75 in 7 cycles, 90 = 90, 115 = 115; S2 / x-line at
  restart 20: 12 in one cycle -> 13 in two.  Both variants (operator applied to the stored column, or
  to the unrounded candidate as the device's delayed DCGS2 does) give those counts;
* under either schedule the float32 basis keeps the float64 basis's counts on every block-Jacobi case:
  the restatement stays inside the +-1 bar the GPU tests use, and the two schedules are within one
  iteration of each other on every line;
* S2 / x-line at restart 20: the float64 basis converges in 12 iterations of ONE cycle, which is a
  reduction the float32 basis cannot carry: the float32 basis needs a second cycle.

Figures (restatement, inner iterations (cycles), float64 -> float32 basis):

    schedule "fixed"   m = 20, 1e-8        m = 5, 1e-8         m = 20, 1e-12
    S2  / BJ(8)        68 (6) -> 68 (6)    69 (17) -> 69 (17)  106 (9) -> 106 (9)
    S4F / BJ(8)        75 (7) -> 75 (7)    90 (22) -> 90 (22)  115 (8) -> 115 (8)
    S2  / x-line 25    12 (1) -> 13 (2)    13 (3) -> 13 (3)    18 (1) -> 25 (2)
    schedule "scipy" (= scipy.sparse.linalg.gmres with the float64 basis)
    S2  / BJ(8)        68 (4) -> 68 (4)    68 (14) -> 68 (14)  105 (6) -> 105 (6)
    S4F / BJ(8)        74 (4) -> 74 (4)    89 (18) -> 89 (18)  114 (6) -> 114 (6)
    S2  / x-line 25    12 (1) -> 14 (2)    13 (3) -> 13 (3)    18 (1) -> 32 (2)
"""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import cbasis_ref as cr
from oracle import arnoldi as ar
from oracle import twin

U32 = 2.0 ** -24      # float32 unit roundoff


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    p = twin.CONFIGS[name]
    csr = twin.generate(p)
    prec = ("bj", 8) if kind == "bj" else ("line", p.shape[-1] if p.dim == 2 else int(np.prod(p.shape[1:])), 25)
    return p, csr, cr.Ops(csr, p.n, prec), twin.rhs(p.n)


RUNS = [(20, 1e-8), (5, 1e-8), (20, 1e-12)]


@functools.lru_cache(maxsize=None)
def _counts(name, kind, m, rtol, basis, variant="rounded", schedule="scipy"):
    p, csr, ops, b = _case(name, kind)
    s = cr.solve_cb(ops.f64, b, rtol=rtol, restart=m, basis=basis, variant=variant, schedule=schedule)
    assert s.info == 0 and s.rnorm <= s.atol_eff
    return s.inner_iters, s.cycles


@pytest.mark.parametrize("m,rtol", RUNS)
@pytest.mark.parametrize("name,kind", [("S2", "bj"), ("S4F", "bj"), ("S2", "line")])
def test_restatement_counts_as_scipy(name, kind, m, rtol):
    """float64 basis: the inner iterations of scipy.sparse.linalg.gmres with the same M."""
    from scipy.sparse.linalg import LinearOperator
    p, (ip, ix, d), ops, b = _case(name, kind)
    A = twin.scipy_csr(ip, ix, np.asarray(d, np.float64), p.n)
    M = LinearOperator((p.n, p.n), matvec=lambda v: ops.f64.Minv(np.asarray(v).reshape(-1)), dtype=np.float64)
    s = twin.scipy_gmres(A, b, M, rtol=rtol, restart=m)
    it, cyc = _counts(name, kind, m, rtol, "float64")
    print(f"{name}/{kind} m={m} rtol={rtol}: SciPy {s.inner_iters}, restatement {it} in {cyc} cycles")
    assert s.info == 0 and it == s.inner_iters


@pytest.mark.parametrize("schedule", ["scipy", "fixed"])
@pytest.mark.parametrize("variant", ["rounded", "candidate"])
@pytest.mark.parametrize("m,rtol", RUNS)
@pytest.mark.parametrize("name", ["S2", "S4F"])
def test_float32_basis_keeps_the_counts(name, m, rtol, variant, schedule):
    f64 = _counts(name, "bj", m, rtol, "float64", "rounded", schedule)
    f32 = _counts(name, "bj", m, rtol, "float32", variant, schedule)
    print(f"{name}/BJ(8) m={m} rtol={rtol} {variant} {schedule}: {f64} -> {f32}")
    assert f64 == f32
    assert abs(f32[0] - _counts(name, "bj", m, rtol, "float32", variant, "scipy")[0]) <= 1, "the schedules differ by more than the bar"


@pytest.mark.parametrize("schedule", ["scipy", "fixed"])
@pytest.mark.parametrize("variant", ["rounded", "candidate"])
def test_xline_pays_one_cycle(variant, schedule):
    f64 = _counts("S2", "line", 20, 1e-8, "float64", "rounded", schedule)
    f32 = _counts("S2", "line", 20, 1e-8, "float32", variant, schedule)
    print(f"S2/x-line m=20 rtol=1e-8 {variant} {schedule}: {f64} -> {f32}")
    assert f64 == (12, 1) and f32[1] == 2 and abs(f32[0] - 13) <= 1


@pytest.mark.parametrize("variant", ["rounded", "candidate"])
def test_issue_table(variant):
    """The table the feature was argued with, entry for entry (SciPy's ptol test against the solve's
    first ptol, schedule "fixed"): 68 = 68 in 6 cycles, 69 = 69, 106 = 106; 75 = 75 in 7 cycles,
    90 = 90, 115 = 115; S2 / x-line at restart 20: 12 in one cycle -> 13 in two; the other x-line
    entries at restart 5 (13 -> 13)."""
    c = functools.partial(_counts, variant=variant, schedule="fixed")
    got = {(n, m, r): (c(n, "bj", m, r, "float64")[0], c(n, "bj", m, r, "float32")[0]) for n in ("S2", "S4F") for m, r in RUNS}
    print(got)
    want = {("S2", 20, 1e-8): (68, 68), ("S2", 5, 1e-8): (69, 69), ("S2", 20, 1e-12): (106, 106),
            ("S4F", 20, 1e-8): (75, 75), ("S4F", 5, 1e-8): (90, 90), ("S4F", 20, 1e-12): (115, 115)}
    assert got == want
    assert (c("S2", "bj", 20, 1e-8, "float64"), c("S4F", "bj", 20, 1e-8, "float64")) == ((68, 6), (75, 7))
    assert (c("S2", "bj", 20, 1e-8, "float32"), c("S4F", "bj", 20, 1e-8, "float32")) == ((68, 6), (75, 7))
    assert (c("S2", "line", 20, 1e-8, "float64"), c("S2", "line", 20, 1e-8, "float32")) == ((12, 1), (13, 2))
    assert (c("S2", "line", 5, 1e-8, "float64")[0], c("S2", "line", 5, 1e-8, "float32")[0]) == (13, 13)


# ---- the restatement's own figures: what sets the GPU bars ----------------------------------------
FIG_CASES = [("S2", "bj", 20), ("S2", "bj", 1), ("S4F", "bj", 20), ("S2", "line", 8)]


@pytest.mark.parametrize("variant", ["rounded", "candidate"])
@pytest.mark.parametrize("name,kind,m", FIG_CASES)
def test_figures_of_a_float32_cycle(name, kind, m, variant):
    """F1-F6 of one full cycle in 80-bit.  What the storage format allows: the start vector is one
    float32 rounding of a unit vector (F3v <= u32), the stored columns are orthonormal and satisfy the
    Arnoldi relation to a small multiple of u32, the correction is the minimiser's to that level; H,
    the rotations, S and beta stay float64 quantities (F3b, F4 at the float64 level)."""
    p, csr, ops, b = _case(name, kind)
    cyc = cr.run_cycle_cb(ops.f64, b, np.zeros(p.n), m, variant=variant)
    f = ar.worst(ar.figures(ops.ld, b, cyc))
    print(f"CBREF|{name}/{kind} m={m} {variant}|" + " ".join(f"{k} {v:.3e}" for k, v in f.items()))
    assert np.array_equal(cyc.V, cyc.V.astype(np.float32).astype(np.float64))
    assert f["F3v"] <= U32 and f["F2"] <= 4 * U32 and f["F1"] <= 4 * U32
    assert f["F3b"] <= 1e-14 and f["F4"] <= 1e-13
    assert 1e-10 < f["F5"] <= 1e-5      # float32-level, not float64-level: the columns were rounded
    f64 = ar.worst(ar.figures(ops.ld, b, cr.run_cycle_cb(ops.f64, b, np.zeros(p.n), m, basis="float64")))
    assert f64["F2"] <= 1e-13 and f64["F1"] <= 1e-13, "the float64 basis of the same code is a float64 Arnoldi"


def test_reference_operators_agree():
    """The product, cyclic and Neumann operators of cbasis_ref in float64 against their 80-bit forms."""
    p = twin.CONFIGS["S2"]
    csr, r = twin.generate(p), twin.rhs(p.n, seed=7)
    for kind in (("product", (32, 25), (1, 8)), ("cyclic", 32, 64), ("neumann", 8, 2)):
        ops = cr.Ops(csr, p.n, kind)
        z, zl = ops.f64.Minv(r), ops.ld.Minv(r)
        assert float(np.linalg.norm((z - zl).astype(np.float64)) / np.linalg.norm(z)) < 1e-12, kind
    # the cyclic lines keep the wrap coupling: M differs from the line-Jacobi M in the wrap entries only
    ip, ix, d = csr
    cyc = cr.Ops(csr, p.n, ("cyclic", 32, 64)).f64
    M = twin.line_matrix(ip, ix, d, p.n, 32, 1 << 40).toarray()
    A = twin.scipy_csr(ip, ix, d, p.n).toarray()
    M[:32, -32:] = A[:32, -32:]
    M[-32:, :32] = A[-32:, :32]
    assert np.allclose(M @ cyc.Minv(r), r, rtol=0, atol=1e-12 * np.abs(r).max())


# ---- ABI and arguments, no device -------------------------------------------------------------------
def test_abi_symbols_and_struct(vk_lib):
    abi = vk_lib._abi
    L = abi.lib()
    for name in ("vtk_gmres_set_basis", "vtk_gmres_basis_info"):
        assert hasattr(L, name) and name in abi.PROTOTYPES
    assert (abi.BASIS_F64, abi.BASIS_F32) == (0, 1) and abi.BASIS == {"float64": 0, "float32": 1}
    assert C.sizeof(abi.BasisInfo) == 24 and abi.BasisInfo.basis_bytes.offset == 8
    assert C.sizeof(abi.Stats) == 80, "vtk_stats keeps its layout"
    assert L.vtk_abi_version() == 6
    with open(abi.HEADER) as f:
        h = f.read()
    assert "VTK_BASIS_F64 = 0, VTK_BASIS_F32 = 1" in h and "int vtk_gmres_set_basis(vtk_ctx *ctx, int basis);" in h
    assert "int32_t requested, used;" in h and "int vtk_gmres_basis_info(vtk_ctx *ctx, vtk_basis_info *out);" in h
    assert L.vtk_gmres_set_basis(None, 1) == abi.ERR_ARG and L.vtk_gmres_basis_info(None, None) == abi.ERR_ARG


@pytest.mark.parametrize("bad", ["float16", "f32", "FLOAT32", 1, np.float32])
def test_bad_basis_raises_before_anything_else(vk_lib, bad):
    """ValueError before any device call: not even the operator is looked at."""
    with pytest.raises(ValueError, match="basis"):
        vk_lib.gmres(object(), None, basis=bad)


# ---- entry layer ----------------------------------------------------------------------------------
def test_vtsetup_basis_node_and_flag(tmp_path, capsys):
    from vtsetup import krylov_precondition as kp
    from vtsetup.config import DEFAULT_XML, Etree, SolverConfig
    assert Etree(DEFAULT_XML).get_node_value("solver/basis") == "float64"
    assert SolverConfig.load().basis == "float64"
    assert SolverConfig.load(basis="float32").basis == "float32"
    with open(DEFAULT_XML) as f:
        xml = f.read()
    on = tmp_path / "on.xml"
    on.write_text(xml.replace("<basis>float64</basis>", "<basis>float32</basis>"))
    assert SolverConfig.load(str(on)).basis == "float32"
    assert SolverConfig.load(str(on), basis="float64").basis == "float64"
    absent = tmp_path / "absent.xml"
    absent.write_text(xml.replace("<basis>float64</basis>", ""))
    assert SolverConfig.load(str(absent)).basis == "float64"
    bad = tmp_path / "bad.xml"
    bad.write_text(xml.replace("<basis>float64</basis>", "<basis>float16</basis>"))
    with pytest.raises(ValueError, match="solver/basis"):
        SolverConfig.load(str(bad))
    for kw in ({"orth": "mgs"}, {"method": "bicgstab"}):
        with pytest.raises(ValueError, match="float32"):
            SolverConfig.load(basis="float32", **kw)
    assert kp.test_main(["--config", "S2", "--basis", "float32", "--dry-run"]) == 0
    assert json.loads(capsys.readouterr().out)["dry_run"] is True
    with pytest.raises(SystemExit):
        kp.test_main(["--config", "S2", "--basis", "float16", "--dry-run"])
    assert kp.test_main(["--config", "S2", "--basis", "float32", "--orth", "mgs", "--dry-run"]) == 2
