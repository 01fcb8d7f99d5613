"""Host-side checks of the two-direction line preconditioner: the definition the
GPU tests' reference rests on, the ABI table, and the vtsetup configuration."""
import re

import numpy as np
import pytest

from oracle import coracle, twin


def _diag_sum(ip, ix, d):
    n = len(ip) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(ip, np.int64)))
    m = np.asarray(ix, np.int64) == rows
    D = np.zeros(n)
    np.add.at(D, rows[m], np.asarray(d)[m].astype(np.float64))
    return D


@pytest.mark.parametrize("segs", [(3, 5), (25, 25), (3, 2)])
def test_definition_on_s4(segs):
    """M1 diag(1/D) M2 = D + X + Y + X D^-1 Y, and its inverse applied to rhs is the chained
    oracle apply line_apply(lf2, D * line_apply(lf1, r)) to 1e-13."""
    p = twin.CONFIGS["S4"]
    ip, ix, d = coracle.generate(p)
    s1, s2 = p.shape[1] * p.shape[2] * p.shape[3], p.shape[2] * p.shape[3]
    M1 = twin.line_matrix(ip, ix, d, p.n, s1, segs[0]).toarray()
    M2 = twin.line_matrix(ip, ix, d, p.n, s2, segs[1]).toarray()
    D = _diag_sum(ip, ix, d)
    assert np.array_equal(np.diag(M1), D) and np.array_equal(np.diag(M2), D)
    X, Y = M1 - np.diag(D), M2 - np.diag(D)
    assert np.count_nonzero(X) and np.count_nonzero(Y)
    M = M1 @ np.diag(1.0 / D) @ M2
    E = np.diag(D) + X + Y + X @ np.diag(1.0 / D) @ Y
    assert np.abs(M - E).max() <= 8 * np.finfo(float).eps * np.abs(E).max()
    r = twin.rhs(p.n)
    z = coracle.line_apply(coracle.line_setup(ip, ix, d, s2, segs[1]),
                           D * coracle.line_apply(coracle.line_setup(ip, ix, d, s1, segs[0]), r))
    zd = np.linalg.solve(M, r)
    assert np.linalg.norm(z - zd) <= 1e-13 * np.linalg.norm(zd)


def test_abi_covers_new_functions(vk_lib):
    abi = vk_lib._abi
    header = open(abi.HEADER).read()
    declared = set(re.findall(r"\b(vtk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert {"vtk_lineproduct_create", "vtk_lineproduct_factors"} <= declared
    assert declared <= set(abi.PROTOTYPES), sorted(declared - set(abi.PROTOTYPES))
    lib = abi.lib()
    for f in ("vtk_lineproduct_create", "vtk_lineproduct_factors"):
        assert getattr(lib, f).argtypes == abi.PROTOTYPES[f][1]
    assert re.search(r"VTK_PREC_LINE2\s*=\s*2", header)
    for name in ("line_product", "LineProduct", "vlasov_line_directions"):
        assert name in vk_lib.__all__ and hasattr(vk_lib, name)


def test_vlasov_line_directions(vk_lib):
    vk = vk_lib
    assert vk.vlasov_line_directions(vk.vlasov_params(1, (100,))) == [1]
    assert vk.vlasov_line_directions(vk.vlasov_params(2, (64, 32))) == [32, 1]
    assert vk.vlasov_line_directions(vk.vlasov_params(4, (6, 5, 8, 7))) == [5 * 8 * 7, 8 * 7]
    for dim, shape in ((1, (100,)), (2, (64, 32)), (4, (200, 125, 50, 40))):
        prm = vk.vlasov_params(dim, shape)
        assert vk.vlasov_line_directions(prm)[0] == vk.vlasov_line_stride(prm)


def test_vtsetup_line_product_config(tmp_path):
    import dataclasses
    from vtsetup.config import DEFAULT_XML, SolverConfig
    base = SolverConfig.load(preconditioner="line_jacobi")
    assert (base.preconditioner, base.line_stride2, base.line_segment2) == ("line_jacobi", 0, 0)
    c = SolverConfig.load(preconditioner="line_product")
    assert c.preconditioner == "line_product" and (c.line_stride2, c.line_segment2) == (0, 0)
    # apart from the type, the same object as the line_jacobi configuration
    assert dataclasses.replace(c, preconditioner="line_jacobi") == base
    xml = open(DEFAULT_XML).read()
    assert "line_stride2" not in xml and "line_product" not in xml   # the packaged file keeps its meaning
    x = tmp_path / "c.xml"
    x.write_text(re.sub(r"<type>\s*\w+\s*</type>", "<type>line_product</type>", xml, count=1).replace(
        "</line_segment>", "</line_segment><line_stride2>64</line_stride2><line_segment2>5</line_segment2>", 1))
    c2 = SolverConfig.load(str(x))
    assert (c2.preconditioner, c2.line_stride2, c2.line_segment2) == ("line_product", 64, 5)
    assert c2.line_segment == base.line_segment and c2.line_stride == base.line_stride
    with pytest.raises(ValueError):
        SolverConfig.load(preconditioner="ilu")
