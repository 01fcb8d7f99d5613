"""Host-side checks of the periodic whole-line preconditioner (vtkrylov.line_cyclic; DESIGN.md
§3m): the definition of M the GPU tests' reference rests on, the ABI table, the vtsetup
configuration and the argument errors that need no device."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import twin


def cyclic_matrix(ip, ix, d, n, stride, period, row0=0):
    """M as a SciPy CSR: of the rows' stored entries (global columns) those on the diagonal and those
    between rows of one cyclic line whose line indices differ by +-1 modulo period; duplicates add
    up in stored order."""
    import scipy.sparse as sp
    rows = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(np.asarray(ip, np.int64))) + row0
    cols = np.asarray(ix, np.int64)
    same_line = (rows % stride == cols % stride) & (rows // (stride * period) == cols // (stride * period))
    di = ((cols // stride) % period - (rows // stride) % period) % period
    keep = (rows == cols) | (same_line & ((di == 1) | (di == period - 1)))
    return sp.csr_matrix((np.asarray(d)[keep].astype(np.float64), (rows[keep] - row0, cols[keep] - row0)),
                         shape=(len(ip) - 1, len(ip) - 1))


@pytest.mark.parametrize("case", ["2d-16-8", "S4-y"])
def test_definition(case):
    """The dense definition, entry by entry, on (16,8) (x-lines: stride Nv, period Nx) and on S4's
    y direction (stride Nvx Nvy, period Ny): M is A's diagonal plus the open whole lines' couplings
    plus, per line, the two wrap couplings between its first and last unknown."""
    if case == "S4-y":
        p = twin.CONFIGS["S4"]
        stride, period = p.shape[2] * p.shape[3], p.shape[1]
    else:
        p = twin.Vlasov(2, (16, 8))
        stride, period = p.shape[1], p.shape[0]
    ip, ix, d = twin.generate(p)
    A = twin.scipy_csr(ip, ix, np.asarray(d, np.float64), p.n).toarray()
    D = np.zeros((p.n, p.n))
    wraps = 0
    for R in range(p.n):
        j, blk, i = R % stride, R // (stride * period), (R // stride) % period
        D[R, R] = A[R, R]
        for di in (-1, 1):
            Rn = (blk * period + (i + di) % period) * stride + j
            D[R, Rn] = A[R, Rn]
            wraps += abs(Rn - R) != stride and A[R, Rn] != 0.0
    M = cyclic_matrix(ip, ix, d, p.n, stride, period).toarray()
    assert np.array_equal(M, D)
    assert np.array_equal(np.diag(M), np.diag(A))
    # the open whole lines (line Jacobi with segments of `period` line indices) and the wrap
    open_lines = twin.line_matrix(ip, ix, np.asarray(d, np.float64), p.n, stride, period).toarray()
    W = M - open_lines
    lines = p.n // period
    assert wraps == 2 * lines and np.count_nonzero(W) == 2 * lines
    r, c = np.nonzero(W)
    assert np.all(np.abs(r - c) == (period - 1) * stride) and np.array_equal(W[r, c], A[r, c])
    # every cyclic line is one irreducible system: period unknowns, 3 entries per row
    assert np.count_nonzero(M) == 3 * p.n


def test_abi_covers_new_functions(vk_lib):
    abi = vk_lib._abi
    header = open(abi.HEADER).read()
    declared = set(re.findall(r"\b(vtk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    new = {"vtk_linecyclic_create", "vtk_linecyclic_info"}
    assert new <= declared
    assert declared <= set(abi.PROTOTYPES), sorted(declared - set(abi.PROTOTYPES))
    lib = abi.lib()
    for f in new:
        assert getattr(lib, f).argtypes == abi.PROTOTYPES[f][1]
    assert abi.PROTOTYPES["vtk_linecyclic_create"][1] == [C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                          C.POINTER(C.c_void_p)]
    assert re.search(r"VTK_PREC_LINEC\s*=\s*3", header)
    # vtk_linec_info as the header lays it out: two int32, three int64, 32 int64
    assert C.sizeof(abi.LinecInfo) == 8 + 3 * 8 + 32 * 8
    for name in ("line_cyclic", "LineCyclic", "vlasov_line_period"):
        assert name in vk_lib.__all__ and hasattr(vk_lib, name)
    for m in ("refresh", "values_epoch", "matvec", "__matmul__", "info", "close"):
        assert hasattr(vk_lib.LineCyclic, m)


def test_vlasov_line_period(vk_lib):
    vk = vk_lib
    assert vk.vlasov_line_period(vk.vlasov_params(1, (100,))) == 100
    assert vk.vlasov_line_period(vk.vlasov_params(2, (64, 32))) == 64
    assert vk.vlasov_line_period(vk.vlasov_params(4, (6, 5, 8, 7))) == 6
    for dim, shape in ((1, (100,)), (2, (64, 32)), (4, (200, 125, 50, 40))):
        prm = vk.vlasov_params(dim, shape)
        assert vk.vlasov_line_stride(prm) * vk.vlasov_line_period(prm) == int(np.prod(shape))


def test_vtsetup_line_cyclic_config(tmp_path):
    import dataclasses
    from vtsetup.config import DEFAULT_XML, SolverConfig
    base = SolverConfig.load(preconditioner="line_jacobi")
    assert base.line_period == 0
    c = SolverConfig.load(preconditioner="line_cyclic")
    assert c.preconditioner == "line_cyclic" and c.line_period == 0
    # apart from the type, the same object as the line_jacobi configuration
    assert dataclasses.replace(c, preconditioner="line_jacobi") == base
    xml = open(DEFAULT_XML).read()
    assert "line_period" not in xml and "line_cyclic" not in xml   # the packaged file keeps its meaning
    x = tmp_path / "c.xml"
    x.write_text(re.sub(r"<type>\s*\w+\s*</type>", "<type>line_cyclic</type>", xml, count=1).replace(
        "</line_segment>", "</line_segment><line_period>64</line_period>", 1))
    c2 = SolverConfig.load(str(x))
    assert (c2.preconditioner, c2.line_period) == ("line_cyclic", 64)
    assert c2.line_segment == base.line_segment and c2.line_stride == base.line_stride
    with pytest.raises(ValueError):
        SolverConfig.load(preconditioner="line_periodic")


def test_argument_errors_without_device(vk_lib):
    """NULL operator / output: VTK_ERR_ARG before anything touches a device; the tuning key exists
    in the header's list."""
    abi = vk_lib._abi
    lib = abi.lib()
    h = C.c_void_p()
    assert lib.vtk_linecyclic_create(None, 8, 16, 4, C.byref(h)) == abi.ERR_ARG
    assert lib.vtk_linecyclic_info(None, None) == abi.ERR_ARG
    assert "linec_serial" in open(abi.HEADER).read()
    with pytest.raises(TypeError):
        vk_lib.line_cyclic()
