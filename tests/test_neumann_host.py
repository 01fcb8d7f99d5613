"""Host-side checks of the Neumann-series wrapper (vtkrylov.neumann): the definition
the GPU tests' reference rests on, the ABI table, the vtsetup element and the argument errors that
need no device.

    N_k^-1 r :  z_1 = M^-1 r ;  z_{i+1} = z_i + M^-1 (r - A z_i),  i = 1 .. k-1
"""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import twin

DEGREES = (1, 2, 3, 4, 8)


def neumann_mv(A, M, degree):
    """The SciPy statement's matvec: A anything with ``@``, M a callable r -> M^-1 r."""
    def mv(r):
        r = np.asarray(r, np.float64).reshape(-1)
        z = M(r)
        for _ in range(degree - 1):
            z = z + M(r - A @ z)
        return z
    return mv


def neumann_operator(A, M, n, degree):
    from scipy.sparse.linalg import LinearOperator
    return LinearOperator((n, n), matvec=neumann_mv(A, M, degree), dtype=np.float64)


def base_matvecs(p, ip, ix, d):
    """name -> M^-1 as a callable, for the bases of the definition test."""
    d64 = np.asarray(d, np.float64)
    Binv = twin.bj_inverse_numpy(ip, ix, d64, p.n, 8)
    stride = p.shape[1] if p.dim == 2 else p.shape[1] * p.shape[2] * p.shape[3]
    lj = twin.line_operator(ip, ix, d64, p.n, stride, 3)
    return {"bj8": lambda r: twin.bj_apply_numpy(Binv, r, p.n), "line3": lj.matvec}


@pytest.mark.parametrize("base", ["bj8", "line3"])
@pytest.mark.parametrize("case", ["16x8", "S4"])
def test_dense_definition(case, base):
    """N_k^-1 = (I - (I - M^-1 A)^k) A^-1 to 1e-12, entry by entry, on (16,8) and S4: the recursion
    applied to the identity's columns against np.linalg.solve."""
    p = twin.Vlasov(2, (16, 8)) if case == "16x8" else twin.CONFIGS["S4"]
    ip, ix, d = twin.generate(p)
    Asp = twin.scipy_csr(ip, ix, np.asarray(d, np.float64), p.n)
    A = Asp.toarray()
    M = base_matvecs(p, ip, ix, d)[base]
    I = np.eye(p.n)
    Minv = np.stack([M(I[:, j]) for j in range(p.n)], axis=1)
    E = I - Minv @ A
    for k in DEGREES:
        mv = neumann_mv(Asp, M, k)
        N = np.stack([mv(I[:, j]) for j in range(p.n)], axis=1)
        ref = np.linalg.solve(A.T, (I - np.linalg.matrix_power(E, k)).T).T    # (I - E^k) A^-1
        err = np.abs(N - ref).max()
        print(f"{case} {base} degree {k}: max |N - (I - E^k) A^-1| = {err:.3e}, max |N| = {np.abs(ref).max():.3e}")
        assert err <= 1e-12, (k, err)
    # degree 1 is the base
    assert np.array_equal(np.stack([neumann_mv(Asp, M, 1)(I[:, j]) for j in range(4)], axis=1), Minv[:, :4])


def test_abi_covers_new_functions(vk_lib):
    abi = vk_lib._abi
    header = open(abi.HEADER).read()
    declared = set(re.findall(r"\b(vtk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    new = {"vtk_neumann_create", "vtk_neumann_info"}
    assert new <= declared
    assert declared <= set(abi.PROTOTYPES), sorted(declared - set(abi.PROTOTYPES))
    lib = abi.lib()
    for f in new:
        assert getattr(lib, f).argtypes == abi.PROTOTYPES[f][1]
    assert abi.PROTOTYPES["vtk_neumann_create"][1] == [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    assert re.search(r"VTK_PREC_NEUMANN\s*=\s*4", header)
    assert abi.PREC_KINDS[4] == "neumann"
    assert C.sizeof(abi.NeuInfo) == 16    # vtk_neu_info: four int32
    for name in ("neumann", "Neumann"):
        assert name in vk_lib.__all__ and hasattr(vk_lib, name)
    for m in ("refresh", "values_epoch", "matvec", "__matmul__", "info", "close"):
        assert hasattr(vk_lib.Neumann, m)
    assert vk_lib.Neumann in vk_lib._PRECS and "Neumann" in vk_lib._PRECS_TEXT
    # the SciPy statement is in the docstring
    assert "z = z + M(r - A @ z)" in vk_lib.Neumann.__doc__
    for key in ("neu_fuse", "neu_dc"):
        assert key in header


def test_argument_errors_without_device(vk_lib):
    """NULL arguments and the degree range: VTK_ERR_ARG before anything touches a device."""
    abi = vk_lib._abi
    lib = abi.lib()
    h = C.c_void_p()
    assert lib.vtk_neumann_create(None, None, 2, C.byref(h)) == abi.ERR_ARG
    assert lib.vtk_neumann_create(None, None, 2, None) == abi.ERR_ARG
    for degree in (0, -1, 9):
        assert lib.vtk_neumann_create(None, None, degree, C.byref(h)) == abi.ERR_ARG
        assert "degree" in abi.last_error()
    assert lib.vtk_neumann_info(None, None) == abi.ERR_ARG
    with pytest.raises(TypeError):
        vk_lib.neumann()
    with pytest.raises(TypeError, match="BlockJacobi"):
        vk_lib.neumann(None, object(), 2)     # the base's type is checked before any handle is read


def test_vtsetup_neumann_degree(tmp_path):
    import dataclasses
    from vtsetup.config import DEFAULT_XML, SolverConfig
    base = SolverConfig.load()
    assert base.neumann_degree == 1
    xml = open(DEFAULT_XML).read()
    assert "neumann" not in xml      # the packaged file keeps its bytes: absent means 1
    x = tmp_path / "c.xml"
    x.write_text(xml.replace("</line_segment>", "</line_segment><neumann_degree>3</neumann_degree>", 1))
    c = SolverConfig.load(str(x))
    assert c.neumann_degree == 3
    assert dataclasses.replace(c, neumann_degree=1) == base
    assert SolverConfig.load(neumann_degree=2, gpus=2).neumann_degree == 2     # run/gpus as for the base kind
    for bad in (0, 9):
        with pytest.raises(ValueError):
            SolverConfig.load(neumann_degree=bad)
    with pytest.raises(ValueError):
        SolverConfig.load(preconditioner="none", neumann_degree=2)
