"""Host-side checks of the cyclic lines that span the ranks (vtkrylov.line_cyclic(..., span=True);
DESIGN.md §3o): the ABI table, the argument errors that need no device, the vtsetup node, and the
NumPy statement of the rank-level algebra -- SPIKE over ranks on open chunks -- against a dense solve
of the cyclic matrix.

The algebra's bar is the preconditioner's own (tests/test_gpu_line_cyclic.py check_apply): with a
longdouble elimination of the cyclic system as the reference and err_ref the error of the float64
dense solve against it, the rank-level solve's error must be <= 16 x max(err_ref, 2^-52 max|x|)."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import twin
from test_line_cyclic_host import cyclic_matrix

LD = np.longdouble


def thomas(a, b, c, r):
    """Open tridiagonal solve, every column one right-hand side (a[0] and c[-1] are not read)."""
    n = len(b)
    u, y = np.array(b, dtype=r.dtype), np.array(r, dtype=r.dtype)
    for i in range(1, n):
        f = a[i] / u[i - 1]
        u[i] = u[i] - f * c[i - 1]
        y[i] = y[i] - f * y[i - 1]
    y[n - 1] = y[n - 1] / u[n - 1]
    for i in range(n - 2, -1, -1):
        y[i] = (y[i] - c[i] * y[i + 1]) / u[i]
    return y


def cyclic_ld(a, b, c, r):
    """The cyclic system in longdouble: the first P - 1 unknowns eliminated, then the last one."""
    a, b, c, r = (np.asarray(v).astype(LD) for v in (a, b, c, r))
    P = len(b)
    e = np.zeros(P - 1, LD)
    e[0] += a[0]
    e[P - 2] += c[P - 2]
    yv = thomas(a[:P - 1], b[:P - 1], c[:P - 1], np.stack([r[:P - 1], e], axis=1))
    y, v = yv[:, 0], yv[:, 1]
    xl = (r[P - 1] - a[P - 1] * y[P - 2] - c[P - 1] * y[0]) / (b[P - 1] - a[P - 1] * v[P - 2] - c[P - 1] * v[0])
    return np.concatenate([y - v * xl, [xl]])


def interface_eliminate(Vf, Vl, Wf, Wl, yf, yl):
    """The interface system as the device solves it (k_linec_span_iface): the chunks merged from
    rank 0 on without pivoting, the cycle closed by a 2 x 2 system, then backwards.  Returns
    (f, l), every rank's first and last unknown."""
    W = len(Vf)
    Yf, Yl, AVf, AVl, AWf, AWl = yf[0], yl[0], Vf[0], Vl[0], Wf[0], Wl[0]
    keep = {}
    for p in range(1, W):
        d = 1.0 / (1.0 - Vf[p] * AWl)
        fa, fb, fc = d * (yf[p] - Vf[p] * Yl), d * (Vf[p] * AVl), -(d * Wf[p])
        la, lb, lc = Yl, AVl, AWl
        keep[p] = (fa, fb, fc, la, lb, lc)
        Yf, AVf, AWf = Yf - AWf * fa, AVf + AWf * fb, AWf * fc
        qa, qb, qc = la - lc * fa, lb + lc * fb, lc * fc
        Yl, AVl, AWl = yl[p] - Vl[p] * qa, -(Vl[p] * qb), Wl[p] - Vl[p] * qc
    m00, m11 = 1.0 + AWf, 1.0 + AVl
    det = m00 * m11 - AVf * AWl
    F, L = (Yf * m11 - AVf * Yl) / det, (m00 * Yl - AWl * Yf) / det
    f, l = np.zeros(W), np.zeros(W)
    f[0], l[W - 1] = F, L
    eta = F
    for p in range(W - 1, 0, -1):
        fa, fb, fc, la, lb, lc = keep[p]
        f[p] = (fa + fb * L) + fc * eta
        l[p - 1] = (la - lb * L) - lc * f[p]
        eta = f[p]
    return f, l


def spike_solve(a, b, c, r, cuts, interface="dense"):
    """One cyclic line (a, b, c, r of P values) solved as DESIGN.md §3o states it: rank p owns the
    indices cuts[p] .. cuts[p + 1]; M_p is its open chunk (the first row's a and the last row's c
    taken as zero), y_p = M_p^-1 r_p, V_p = M_p^-1 (a_first e_first), W_p = M_p^-1 (c_last e_last);
    the interface unknowns (every rank's first and last) from
        l_{p-1} + V_{p-1,last} l_{p-2} + W_{p-1,last} f_p = y_{p-1,last}
        f_p + V_{p,first} l_{p-1} + W_{p,first} f_{p+1} = y_{p,first}
    (numpy.linalg.solve, or the device's elimination); x_p = y_p - V_p xi_p - W_p eta_p."""
    W = len(cuts) - 1
    y, V, Wk = [], [], []
    for p in range(W):
        s = slice(cuts[p], cuts[p + 1])
        n = cuts[p + 1] - cuts[p]
        ef, el = np.zeros(n), np.zeros(n)
        ef[0], el[-1] = a[s][0], c[s][-1]
        sol = thomas(a[s], b[s], c[s], np.stack([r[s], ef, el], axis=1))
        y.append(sol[:, 0]); V.append(sol[:, 1]); Wk.append(sol[:, 2])
    Vf, Vl = np.array([v[0] for v in V]), np.array([v[-1] for v in V])
    Wf, Wl = np.array([w[0] for w in Wk]), np.array([w[-1] for w in Wk])
    yf, yl = np.array([v[0] for v in y]), np.array([v[-1] for v in y])
    if interface == "dense":   # unknown 2 p: f_p, 2 p + 1: l_p
        K, g = np.zeros((2 * W, 2 * W)), np.zeros(2 * W)
        for p in range(W):
            lm, fn = 2 * ((p - 1) % W) + 1, 2 * ((p + 1) % W)
            K[2 * p, 2 * p] += 1.0; K[2 * p, lm] += Vf[p]; K[2 * p, fn] += Wf[p]; g[2 * p] = yf[p]
            K[2 * p + 1, 2 * p + 1] += 1.0; K[2 * p + 1, lm] += Vl[p]; K[2 * p + 1, fn] += Wl[p]; g[2 * p + 1] = yl[p]
        u = np.linalg.solve(K, g)
        f, l = u[0::2], u[1::2]
    else:
        f, l = interface_eliminate(Vf, Vl, Wf, Wl, yf, yl)
    return np.concatenate([y[p] - V[p] * l[(p - 1) % W] - Wk[p] * f[(p + 1) % W] for p in range(W)])


@pytest.mark.parametrize("interface", ["dense", "eliminate"])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", [(16, 8), (50, 8)])
def test_rank_level_algebra(vk_lib, shape, world, interface):
    p = twin.Vlasov(2, shape)
    stride, period = shape[1], shape[0]
    ip, ix, d = twin.generate(p)
    M = cyclic_matrix(ip, ix, d, p.n, stride, period).toarray()
    r = twin.rhs(p.n)
    cuts = [int(v) // stride for v in vk_lib.partition_rows(p.n, world, stride)]
    assert cuts[0] == 0 and cuts[-1] == period and min(np.diff(cuts)) >= 3, cuts
    xd = np.linalg.solve(M, r)
    x, xl = np.zeros(p.n), np.zeros(p.n, LD)
    R = np.arange(period) * stride
    for j in range(stride):
        rows = R + j
        a = M[rows, np.roll(rows, 1)]
        b = M[rows, rows]
        c = M[rows, np.roll(rows, -1)]
        x[rows] = spike_solve(a, b, c, r[rows], cuts, interface)
        xl[rows] = cyclic_ld(a, b, c, r[rows])
    err_ref = float(np.abs(xd.astype(LD) - xl).max())
    err = float(np.abs(x.astype(LD) - xl).max())
    floor = 2.0 ** -52 * float(np.abs(xl).max())
    print(f"{shape} world {world} {interface}: error {err:.3e}, dense solve's {err_ref:.3e}, 2^-52 max|x| {floor:.3e}")
    assert err <= 16 * max(err_ref, floor), (err, err_ref, floor)


def test_abi_covers_span_functions(vk_lib):
    abi = vk_lib._abi
    header = open(abi.HEADER).read()
    declared = set(re.findall(r"\b(vtk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    new = {"vtk_linecyclic_create_span", "vtk_linecyclic_span_info"}
    assert new <= declared
    assert declared <= set(abi.PROTOTYPES), sorted(declared - set(abi.PROTOTYPES))
    lib = abi.lib()
    for f in new:
        assert getattr(lib, f).argtypes == abi.PROTOTYPES[f][1]
    assert abi.PROTOTYPES["vtk_linecyclic_create_span"][1] == [C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                               C.POINTER(C.c_void_p)]
    assert abi.PROTOTYPES["vtk_linecyclic_span_info"][1] == [C.c_void_p, C.c_void_p]
    # vtk_linec_span_info as the header lays it out: four int32, three int64
    assert C.sizeof(abi.LinecSpanInfo) == 4 * 4 + 3 * 8
    assert re.search(r"VTK_ABI_VERSION\s+6\b", header) and abi.ABI_VERSION == 6
    assert hasattr(vk_lib.LineCyclic, "span_info")
    import inspect
    assert inspect.signature(vk_lib.line_cyclic).parameters["span"].default is False


def test_argument_errors_without_device(vk_lib):
    abi = vk_lib._abi
    lib = abi.lib()
    h = C.c_void_p()
    assert lib.vtk_linecyclic_create_span(None, 8, 16, 4, C.byref(h)) == abi.ERR_ARG
    assert lib.vtk_linecyclic_span_info(None, None) == abi.ERR_ARG


def test_vtsetup_line_span_config(tmp_path):
    from vtsetup.config import DEFAULT_XML, SolverConfig
    c = SolverConfig.load(preconditioner="line_cyclic")
    assert c.line_span == 0
    assert SolverConfig.load(preconditioner="line_cyclic", line_span=1).line_span == 1
    xml = open(DEFAULT_XML).read()
    assert "line_span" not in xml   # the packaged file keeps its meaning
    x = tmp_path / "c.xml"
    x.write_text(re.sub(r"<type>\s*\w+\s*</type>", "<type>line_cyclic</type>", xml, count=1).replace(
        "</line_segment>", "</line_segment><line_span>1</line_span>", 1))
    assert SolverConfig.load(str(x)).line_span == 1
    with pytest.raises(ValueError):
        SolverConfig.load(preconditioner="line_cyclic", line_span=2)
    with pytest.raises(ValueError):
        SolverConfig.load(preconditioner="line_cyclic", line_span=1, neumann_degree=2)
    for kind in ("line_jacobi", "block_jacobi", "none"):   # it would be ignored: refused instead
        with pytest.raises(ValueError, match="line_span"):
            SolverConfig.load(preconditioner=kind, line_span=1)
