"""vtkrylov — MI355X-native preconditioned Krylov path (CSR SpMV + block-Jacobi + GMRES).

Drop-in for the north_star's "reference scipy.sparse path" (SURVEY.md §8b): the callables
below keep SciPy's names, argument meaning and error behaviour, and route every operation to
the gfx950 kernels of ``libvtkrylov.so`` through the C-ABI in ``include/vtkrylov.h``.

    scipy.sparse.csr_matrix((data, indices, indptr), shape)  ->  vtkrylov.csr_matrix(...)
    A @ x                                                    ->  A @ x   (vtk_spmv)
    LinearOperator(matvec=block-Jacobi)                      ->  vtkrylov.block_jacobi(A, bs)
    scipy.sparse.linalg.gmres(A, b, x0, rtol=, atol=,        ->  vtkrylov.gmres(...)
                              restart=, maxiter=, M=)           (iterative.py:582-841)
    scipy.sparse.linalg.bicgstab(A, b, x0, rtol=, atol=,     ->  vtkrylov.bicgstab(...)
                                 maxiter=, M=)                  (seven work vectors; 1-8 ranks)

Vectors may be NumPy arrays (host; copied in and out) or torch CUDA tensors (device memory,
used in place).  There is no CPU fallback: without the library or a HIP device every call
raises.
"""
from __future__ import annotations

import atexit
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _abi
from ._abi import check, lib

__all__ = ["Context", "default_context", "csr_matrix", "load_npz", "save_npz", "vlasov_operator", "block_jacobi",
           "gmres", "VlasovParams", "vlasov_params", "rhs_splitmix", "partition_rows",
           "halo_plan", "device_count", "SolveStats", "line_jacobi", "LineJacobi", "line_product", "LineProduct", "line_cyclic", "LineCyclic",
           "neumann", "Neumann",
           "vlasov_line_period",
           "vlasov_line_directions",
           "vlasov_line_stride", "bicgstab", "BicgstabStats", "last_bicgstab_stats",
           "ArnoldiCapture", "last_arnoldi", "BasisInfo", "last_basis_info"]

VlasovParams = _abi.VlasovParams

# At interpreter exit the finalizers below may run in any order (a context before the operators
# that use it); the process is ending, so they leave the native objects to the runtime.
_exiting = [False]
atexit.register(lambda: _exiting.__setitem__(0, True))


def vlasov_params(dim: int, shape, *, fp32=False, vmax=6.0, E0=0.5, nu=0.05, alpha=0.25,
                  cfl=4.0) -> VlasovParams:
    s = list(shape) + [0] * (4 - len(shape))
    return VlasovParams(int(dim), int(bool(fp32)), (C.c_int64 * 4)(*s), vmax, E0, nu, alpha, cfl)


def device_count() -> int:
    n = C.c_int()
    lib().vtk_device_count(C.byref(n))
    return n.value


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_torch_cuda(x) -> bool:
    t = type(x)
    return t.__module__.startswith("torch") and getattr(x, "is_cuda", False)


class _Vec:
    """A vector argument: NumPy (host, kind=HOST) or torch CUDA tensor (device, kind=DEVICE)."""

    def __init__(self, x, n: int, writable=False):
        if _is_torch_cuda(x):
            import torch
            if x.dtype != torch.float64 or not x.is_contiguous() or x.numel() != n:
                raise ValueError("device vectors must be contiguous float64 tensors of length n")
            torch.cuda.current_stream(x.device).synchronize()
            self.kind = _abi.PTR_DEVICE
            self.ptr = C.c_void_p(x.data_ptr())
            self.obj = x
        else:
            a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"vector has length {a.shape[0]}, expected {n}")
            if writable and not a.flags.writeable:
                a = a.copy()
            self.kind = _abi.PTR_HOST
            self.ptr = _np_ptr(a)
            self.obj = a


class Context:
    """One HIP device + stream (+ optional RCCL communicator).  ``vtk_ctx_create``."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib().vtk_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = device
        self.rank, self.world = 0, 1

    @property
    def handle(self):
        return self._h

    def stream_ptr(self) -> int:
        s = C.c_void_p()
        check(lib().vtk_ctx_stream(self._h, C.byref(s)), self._h)
        return s.value or 0

    def synchronize(self):
        check(lib().vtk_ctx_synchronize(self._h), self._h)

    def comm_init(self, rank: int, world: int, unique_id: bytes | None):
        buf = None if unique_id is None else C.create_string_buffer(bytes(unique_id), 128)
        check(lib().vtk_comm_init(self._h, rank, world, buf), self._h)
        self.rank, self.world = rank, world

    def rccl_ranks(self) -> int:
        """Ranks of the RCCL communicator (ncclCommCount); 0 without one."""
        n = C.c_int()
        check(lib().vtk_comm_rccl_count(self._h, C.byref(n)), self._h)
        return n.value

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        check(lib().vtk_comm_unique_id(buf))
        return buf.raw

    def comm_init_host(self, rank: int, world: int, group=None):
        """Host-staged communicator over torch.distributed (tests; ranks may share a GPU)."""
        from .comm import init_host
        return init_host(self, rank, world, group)

    def profile(self, on: bool = True):
        """Enable (and clear) / disable the per-kernel-class event profile."""
        check(lib().vtk_profile_enable(self._h, int(bool(on))), self._h)

    def profile_read(self) -> dict:
        """{class: {launches, seconds, bytes, avg_us, gbs}} from the event profile."""
        n = C.c_int()
        check(lib().vtk_profile_read(self._h, None, 0, C.byref(n)), self._h)
        arr = (_abi.KernelProfile * max(n.value, 1))()
        check(lib().vtk_profile_read(self._h, arr, n.value, C.byref(n)), self._h)
        out = {}
        for e in arr[:n.value]:
            if e.launches:
                out[e.name.decode()] = {"launches": e.launches, "seconds": e.seconds, "bytes": e.bytes,
                                        "avg_us": e.seconds / e.launches * 1e6,
                                        "gbs": e.bytes / e.seconds / 1e9 if e.seconds > 0 else 0.0}
        return out

    orth = _abi.ORTH_AUTO

    def set_orth(self, orth: int):
        check(lib().vtk_gmres_set_orth(self._h, int(orth)), self._h)
        self.orth = int(orth)

    basis = _abi.BASIS_F64

    def set_basis(self, basis: int):
        """Storage of the Krylov basis in :func:`gmres` (``vtk_gmres_set_basis``):
        ``_abi.BASIS_F64`` (default) or ``_abi.BASIS_F32``, the compressed basis."""
        check(lib().vtk_gmres_set_basis(self._h, int(basis)), self._h)
        self.basis = int(basis)

    def basis_info(self) -> "BasisInfo":
        o = _abi.BasisInfo()
        check(lib().vtk_gmres_basis_info(self._h, C.byref(o)), self._h)
        return BasisInfo(requested=int(o.requested), used=int(o.used), basis_bytes=int(o.basis_bytes),
                         workspace_bytes=int(o.workspace_bytes))

    def set_tuning(self, key: str, value: int):
        """A/B and test switch of this context (``vtk_ctx_set_tuning``; keys in
        include/vtkrylov.h).  Seeded from ``VTK_<KEY>`` when the context was created."""
        check(lib().vtk_ctx_set_tuning(self._h, key.encode(), int(value)), self._h)

    def get_tuning(self, key: str) -> int:
        v = C.c_int()
        check(lib().vtk_ctx_get_tuning(self._h, key.encode(), C.byref(v)), self._h)
        return v.value

    def tuning(self, **kv):
        """``with ctx.tuning(band_lsv=0): ...`` -- set switches for a block, then restore."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_tuning(k) for k in kv}
            try:
                for k, v in kv.items():
                    self.set_tuning(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_tuning(k, v)
        return cm()

    def capture_arnoldi(self, cycle: int = 0):
        """``with ctx.capture_arnoldi(0): vk.gmres(...)`` -- a test hook: the solves of the block
        copy restart cycle ``cycle`` (0-based; -2: the last cycle run) aside for
        :func:`last_arnoldi` (``vtk_gmres_capture``).  Disarmed on exit."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            check(lib().vtk_gmres_capture(self._h, int(cycle)), self._h)
            try:
                yield self
            finally:
                check(lib().vtk_gmres_capture(self._h, -1), self._h)
        return cm()

    band = True

    def set_band(self, on: bool):
        """Allow (default) or forbid the line-band DCGS2 step (see csr_matrix.set_line_band)."""
        check(lib().vtk_gmres_set_band(self._h, 1 if on else 0), self._h)
        self.band = bool(on)

    def close(self):
        if getattr(self, "_h", None):
            lib().vtk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        if _exiting[0]:
            return
        try:
            self.close()
        except Exception:
            pass


_default = {}


def default_context(device: int = 0) -> Context:
    if device not in _default:
        _default[device] = Context(device)
    return _default[device]


class CsrOperator:
    """Device-resident CSR operator (this rank's row block).  ``vtk_csr_create``."""

    def __init__(self, handle, ctx: Context, fp32: bool):
        self._h = handle
        self.ctx = ctx
        self.fp32 = bool(fp32)
        ng, rb, re_, nnz, nh = (C.c_int64() for _ in range(5))
        check(lib().vtk_csr_info(handle, C.byref(ng), C.byref(rb), C.byref(re_), C.byref(nnz),
                                 C.byref(nh)), ctx.handle)
        self.n_global, self.row_begin, self.row_end = ng.value, rb.value, re_.value
        self.nnz, self.n_halo = nnz.value, nh.value
        self.n_local = self.row_end - self.row_begin
        self.shape = (self.n_global, self.n_global)
        self.dtype = np.dtype(np.float64)

    @property
    def handle(self):
        return self._h

    LAYOUTS = {"auto": 0, "csr": 1, "sell": 2, "sell32": 3}

    def set_layout(self, layout: str):
        """SpMV layout: "sell" (SELL-64 copy, columns dictionary-coded per 64-row chunk),
        "sell32" (SELL-64 with int32 columns), "csr" (CSR-stream tiles) or "auto" ("sell" when
        its padding is <= 25 % of nnz).  Results are bit-identical in every layout."""
        check(lib().vtk_csr_set_layout(self._h, self.LAYOUTS[layout]), self.ctx.handle)

    @property
    def layout(self) -> str:
        v = C.c_int()
        check(lib().vtk_csr_get_layout(self._h, C.byref(v)), self.ctx.handle)
        return {1: "csr", 2: "sell", 3: "sell32"}[v.value]

    def set_line_band(self, line_len: int):
        """Declare the line-band structure: rows form x-lines of ``line_len`` rows and every
        column lies in the lines x-1..x+1 (periodic) of its row's line (checked on the device;
        0 clears it).  The 2D Vlasov operators get it automatically (line_len = Nv).  gmres then
        fuses each DCGS2 update pass with the next step's SpMV + BJ + dots (one basis read per
        step); results stay within the DCGS2 bars."""
        check(lib().vtk_csr_set_line_band(self._h, int(line_len)), self.ctx.handle)

    @property
    def line_band(self) -> int:
        v = C.c_int64()
        check(lib().vtk_csr_get_line_band(self._h, C.byref(v)), self.ctx.handle)
        return v.value

    @property
    def line_separable(self) -> bool:
        """True when the band step reads the values from per-position / per-line tables (the
        operator's x couplings depend only on v, its v couplings only on x; checked bit for bit
        when the band was set -- vtk_csr_get_line_values)."""
        return self.line_values > 0

    @property
    def line_values(self) -> int:
        """0: SELL values; 1: line-separable values; 2: also canonical rows (no column codes read
        by the band step) -- vtk_csr_get_line_values."""
        v = C.c_int()
        check(lib().vtk_csr_get_line_values(self._h, C.byref(v)), self.ctx.handle)
        return v.value

    def set_grid4(self, Ny: int, Nvx: int, Nvy: int):
        """Declare the 4D phase-space grid structure (vtk_csr_set_grid4; checked on the device, Ny 0
        clears it).  The 4D Vlasov operators get it automatically, also when uploaded as a CSR."""
        check(lib().vtk_csr_set_grid4(self._h, int(Ny), int(Nvx), int(Nvy)), self.ctx.handle)

    @property
    def grid4(self) -> tuple:
        """(Ny, Nvx, Nvy) of the verified 4D grid structure, (0, 0, 0) when not set."""
        v = (C.c_int64 * 3)()
        check(lib().vtk_csr_get_grid4(self._h, v), self.ctx.handle)
        return tuple(int(t) for t in v)

    def layout_info(self) -> dict:
        """Layout in use, bytes of the operator one SpMV reads in it, SELL chunk counts."""
        li = _abi.LayoutInfo()
        check(lib().vtk_csr_layout_info(self._h, C.byref(li)), self.ctx.handle)
        d = {k: getattr(li, k) for k, _ in li._fields_}
        d["layout"] = {1: "csr", 2: "sell", 3: "sell32"}[d["layout"]]
        return d

    def matvec(self, x):
        """y = A x on this rank's rows (sparsetools csr_matvec, bit-identical)."""
        vx = _Vec(x, self.n_local)
        if vx.kind == _abi.PTR_DEVICE:
            import torch
            y = torch.empty_like(vx.obj)
            check(lib().vtk_spmv(self._h, vx.ptr, C.c_void_p(y.data_ptr()), vx.kind), self.ctx.handle)
            self.ctx.synchronize()
            return y
        y = np.empty(self.n_local)
        check(lib().vtk_spmv(self._h, vx.ptr, _np_ptr(y), vx.kind), self.ctx.handle)
        return y

    def __matmul__(self, x):
        return self.matvec(x)

    def dot(self, x):
        return self.matvec(x)

    def precond_matvec(self, M, x):
        """w = M^-1 (A x) through the launch the solver's split DCGS2 step uses for this operator
        (SciPy: ``M.matvec(A @ x)``; vtk_precond_matvec).  M: a BlockJacobi / LineJacobi /
        LineProduct of this operator, or None (w = A x)."""
        if M is not None and not isinstance(M, _PRECS):
            raise TypeError("CsrOperator.precond_matvec: M must be " + _PRECS_TEXT)
        vx = _Vec(x, self.n_local)
        mh = M.handle if M is not None else None
        if vx.kind == _abi.PTR_DEVICE:
            import torch
            w = torch.empty_like(vx.obj)
            check(lib().vtk_precond_matvec(self._h, mh, vx.ptr, C.c_void_p(w.data_ptr()), vx.kind), self.ctx.handle)
            self.ctx.synchronize()
            return w
        w = np.empty(self.n_local)
        check(lib().vtk_precond_matvec(self._h, mh, vx.ptr, _np_ptr(w), vx.kind), self.ctx.handle)
        return w

    def download(self):
        """(indptr, indices[global], data) of this rank's rows, as stored on the device."""
        ip = np.empty(self.n_local + 1, np.int32)
        ix = np.empty(max(self.nnz, 1), np.int32)
        d = np.empty(max(self.nnz, 1), np.float32 if self.fp32 else np.float64)
        check(lib().vtk_csr_download(self._h, _np_ptr(ip), _np_ptr(ix), _np_ptr(d)), self.ctx.handle)
        return ip, ix[:self.nnz], d[:self.nnz]

    def update_values(self, data):
        """SciPy's ``A.data[:] = data``: replace the values, keep the sparsity pattern
        (``vtk_csr_update_values``).  ``data``: ``nnz`` values in the order of
        :func:`csr_matrix` / :meth:`download` -- a NumPy array or a torch tensor on the context's
        device, float32 for an fp32 operator, else float64 (anything else: ValueError, before any
        device work).  Afterwards the operator equals one freshly built from these values;
        preconditioners keep their old factors until their ``refresh()``."""
        want = np.float32 if self.fp32 else np.float64
        if _is_device(data):
            import torch
            if data.dtype != (torch.float32 if self.fp32 else torch.float64):
                raise ValueError(f"update_values: dtype {data.dtype}, the operator stores {np.dtype(want).name}")
            if data.dim() != 1 or data.numel() != self.nnz:
                raise ValueError(f"update_values: {tuple(data.shape)} values given, the operator has nnz = {self.nnz}")
            if data.device.index != self.ctx.device:
                raise ValueError(f"update_values: tensor on {data.device}, the context is on cuda:{self.ctx.device}")
            data = data.contiguous()
            # the library copies on its own stream: the tensor must be complete first
            torch.cuda.current_stream(data.device).synchronize()
            check(lib().vtk_csr_update_values(self._h, C.c_void_p(data.data_ptr()), _abi.PTR_DEVICE),
                  self.ctx.handle)
            return self
        a = np.asarray(data)
        if a.dtype != want:
            raise ValueError(f"update_values: dtype {a.dtype}, the operator stores {np.dtype(want).name}")
        if a.ndim != 1 or a.shape[0] != self.nnz:
            raise ValueError(f"update_values: {a.shape} values given, the operator has nnz = {self.nnz}")
        a = np.ascontiguousarray(a)
        check(lib().vtk_csr_update_values(self._h, _np_ptr(a), _abi.PTR_HOST), self.ctx.handle)
        return self

    def update_vlasov(self, params: VlasovParams):
        """The same for an operator made by :func:`vlasov_operator`: regenerate the values from
        ``params`` on the device (``vtk_csr_update_vlasov``).  dim, shape and fp32 must be the
        creating ones; vmax, E0, nu, alpha and cfl may change."""
        check(lib().vtk_csr_update_vlasov(self._h, C.byref(params)), self.ctx.handle)
        return self

    @property
    def values_epoch(self) -> int:
        """Number of successful value updates (0 after creation)."""
        e = C.c_int64()
        check(lib().vtk_csr_values_epoch(self._h, C.byref(e)), self.ctx.handle)
        return e.value

    def close(self):
        if getattr(self, "_h", None):
            lib().vtk_csr_destroy(self._h)
            self._h = None

    def __del__(self):
        if _exiting[0]:
            return
        try:
            self.close()
        except Exception:
            pass


def _is_device(a) -> bool:
    return getattr(a, "is_cuda", False) is True


def _apply_line_len(A: CsrOperator, line_len):
    """line_len None: keep what vtk_csr_create detected (the 2D Vlasov x-lines are found in
    the CSR itself); 0: no line band; L: require the line band of L rows (ValueError if the
    operator does not have it)."""
    if line_len is None:
        return A
    if int(line_len) != A.line_band:
        A.set_line_band(int(line_len))
    return A


def csr_matrix(arg, shape=None, *, ctx: Context | None = None, offsets=None, line_len=None) -> CsrOperator:
    """Build a device CSR operator from ``(data, indices, indptr)`` or a SciPy sparse matrix.

    With ``offsets`` (world+1 row boundaries) the arrays are this rank's row block with
    global column indices (multi-GPU); otherwise the whole matrix.  The library looks for the
    x-line structure of the 2D Vlasov operators in the CSR (``line_len=None``, the default) and
    then runs the same fused solver as for a generated operator; ``line_len=0`` turns that off,
    an explicit ``line_len`` requires it (see :meth:`CsrOperator.set_line_band`)."""
    ctx = ctx or default_context()
    if hasattr(arg, "tocsr"):
        # stored order kept: csr_matvec sums each row in stored order, so must the device
        m = arg.tocsr()
        data, indices, indptr = m.data, m.indices, m.indptr
        shape = m.shape
    else:
        data, indices, indptr = arg
    if shape is None or shape[0] != shape[1]:
        raise ValueError("a square shape is required")
    if _is_device(data) or _is_device(indices) or _is_device(indptr):
        # CSR already in HBM (torch tensors on the context's device): no host round trip; the
        # library validates indptr (host copy) and the column range (device reduction)
        import torch
        if not (_is_device(data) and _is_device(indices) and _is_device(indptr)):
            raise TypeError("csr_matrix: data, indices and indptr must all be device tensors or all host arrays")
        for t in (data, indices, indptr):
            if t.device.index != ctx.device:
                raise ValueError(f"csr_matrix: tensor on {t.device}, the context is on cuda:{ctx.device}")
        fp32 = data.dtype == torch.float32
        data = data.contiguous().to(torch.float32 if fp32 else torch.float64)
        indices = indices.contiguous().to(torch.int32)
        indptr = indptr.contiguous().to(torch.int32)
        # the conversions above run on torch's current stream; the library copies with
        # hipMemcpy on its own: let them finish first
        torch.cuda.current_stream(data.device).synchronize()
        nnz = int(indptr[-1].item())   # the CSR may carry spare capacity beyond indptr[-1]
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
        # the library copies nnz entries device to device: never past the tensors' ends
        n_rows = int(shape[0]) if offs is None else int(offs[ctx.rank + 1] - offs[ctx.rank])
        if indptr.numel() != n_rows + 1:
            raise ValueError(f"csr_matrix: indptr has {indptr.numel()} entries, expected {n_rows + 1}")
        if nnz < 0 or nnz > indices.numel() or nnz > data.numel():
            raise ValueError(f"csr_matrix: indptr[-1] = {nnz} exceeds the {indices.numel()} indices / "
                             f"{data.numel()} values given")
        h = C.c_void_p()
        check(lib().vtk_csr_create(ctx.handle, int(shape[0]), None if offs is None else _np_ptr(offs),
                                   nnz, C.c_void_p(indptr.data_ptr()),
                                   C.c_void_p(indices.data_ptr()), C.c_void_p(data.data_ptr()),
                                   int(fp32), _abi.PTR_DEVICE, C.byref(h)), ctx.handle)
        return _apply_line_len(CsrOperator(h, ctx, fp32), line_len)
    data = np.asarray(data)
    fp32 = data.dtype == np.float32
    data = np.ascontiguousarray(data, dtype=np.float32 if fp32 else np.float64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    nnz = int(indptr[-1])
    n_rows = int(shape[0]) if offs is None else int(offs[ctx.rank + 1] - offs[ctx.rank])
    if indptr.shape[0] != n_rows + 1:
        raise ValueError(f"csr_matrix: indptr has {indptr.shape[0]} entries, expected {n_rows + 1}")
    if nnz < 0 or nnz > indices.shape[0] or nnz > data.shape[0]:
        raise ValueError(f"csr_matrix: indptr[-1] = {nnz} exceeds the {indices.shape[0]} indices / "
                         f"{data.shape[0]} values given")
    h = C.c_void_p()
    check(lib().vtk_csr_create(ctx.handle, int(shape[0]), None if offs is None else _np_ptr(offs),
                               nnz, _np_ptr(indptr), _np_ptr(indices), _np_ptr(data),
                               int(fp32), _abi.PTR_HOST, C.byref(h)), ctx.handle)
    return _apply_line_len(CsrOperator(h, ctx, fp32), line_len)


def load_npz(file, *, ctx: Context | None = None, offsets=None, line_len=None) -> CsrOperator:
    """``scipy.sparse.load_npz`` for CSR archives, straight to the device: with ``offsets``
    (world+1 row boundaries) each rank reads only its row block (``ctx.rank``).  ``line_len``
    as in :func:`csr_matrix`."""
    from .npz import load_npz_arrays
    ctx = ctx or default_context()
    rows = None
    if offsets is not None:
        offs = np.asarray(offsets, dtype=np.int64)
        if offs.shape != (ctx.world + 1,):
            raise ValueError("offsets must have world+1 entries")
        rows = (int(offs[ctx.rank]), int(offs[ctx.rank + 1]))
    indptr, indices, data, shape = load_npz_arrays(file, rows)
    return csr_matrix((data, indices, indptr), shape=shape, ctx=ctx, offsets=offsets, line_len=line_len)


def save_npz(file, A: CsrOperator, compressed: bool = True) -> None:
    """``scipy.sparse.save_npz`` of a whole (single-rank) device operator, entries in stored
    order; a row-sharded operator is saved per rank with ``npz.save_npz_arrays`` on
    ``A.download()`` (global column ids) and concatenated by the caller."""
    from .npz import save_npz_arrays
    if A.n_local != A.n_global:
        raise ValueError("save_npz needs the whole matrix on this rank (row-sharded operator)")
    indptr, indices, data = A.download()
    save_npz_arrays(file, indptr, indices, data, A.shape, compressed)


def vlasov_operator(params: VlasovParams, *, ctx: Context | None = None, offsets=None) -> CsrOperator:
    """Generate the Appendix-A Vlasov operator directly in device memory."""
    ctx = ctx or default_context()
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    h = C.c_void_p()
    check(lib().vtk_csr_create_vlasov(ctx.handle, C.byref(params),
                                      None if offs is None else _np_ptr(offs), C.byref(h)), ctx.handle)
    return CsrOperator(h, ctx, bool(params.fp32))


BJ_MODES = {"auto": 0, "inverse": 1, "tridiag": 2}


def _refresh(M):
    e = C.c_int64(M._epoch)
    try:
        check(lib().vtk_prec_refresh(M._h, C.byref(e)), M.A.ctx.handle)
    finally:
        M._epoch = e.value   # written by the library once the factors are whole (also on ValueError)
    return M


class _Prec:
    """What the preconditioner classes share: the handle and its release, the apply, the epoch of
    the values the factors were computed from."""

    def _adopt(self, h, A: "CsrOperator", epoch: int):
        self._h = h
        self.A = A
        self.shape = A.shape
        self.dtype = np.dtype(np.float64)
        self._epoch = epoch

    @property
    def values_epoch(self) -> int:
        """``A.values_epoch`` of the values the factors were computed from."""
        return self._epoch

    @property
    def handle(self):
        return self._h

    def matvec(self, r):
        vr = _Vec(r, self.A.n_local)
        if vr.kind == _abi.PTR_DEVICE:
            import torch
            z = torch.empty_like(vr.obj)
            check(lib().vtk_prec_apply(self._h, vr.ptr, C.c_void_p(z.data_ptr()), vr.kind), self.A.ctx.handle)
            self.A.ctx.synchronize()
            return z
        z = np.empty(self.A.n_local)
        check(lib().vtk_prec_apply(self._h, vr.ptr, _np_ptr(z), vr.kind), self.A.ctx.handle)
        return z

    def __matmul__(self, r):
        return self.matvec(r)

    def close(self):
        if getattr(self, "_h", None):
            lib().vtk_prec_destroy(self._h)
            self._h = None

    def __del__(self):
        if _exiting[0]:
            return
        try:
            self.close()
        except Exception:
            pass


class BlockJacobi(_Prec):
    """Block-Jacobi preconditioner M = blockdiag(A)^-1 (SciPy: a LinearOperator whose matvec
    applies the bs x bs diagonal-block inverses).  ``vtk_bjacobi_create``.

    ``mode``: how M^-1 is applied (same operator either way): "inverse" multiplies by the
    block inverses (bit-identical to the oracle with setup "exact"), "tridiag" solves with the LU factors of
    tridiagonal blocks (bs 2/4/8; 24 B/row instead of 8*bs), "auto" (default) takes "tridiag"
    when every block is tridiagonal and its factors pass the setup check.

    ``setup``: how the inverses are computed: "exact" (default, as ``vtk_bjacobi_create``:
    Gauss-Jordan with partial pivoting, bit-identical to the oracle), "mfma" (bs 16 / 32: blocked
    Gauss-Jordan with the rank-4 panel updates on the fp64 matrix cores; same pivot rule,
    rounding-level differences) or "auto" ("mfma" for bs 16 and 32, 2.3x / 4.7x faster at C3,
    else "exact")."""

    SETUPS = {"exact": 0, "mfma": 1, "auto": 2}

    def __init__(self, A: CsrOperator, bs: int = 8, mode: str = "auto", setup: str = "exact"):
        if mode not in BJ_MODES:
            raise ValueError(f"mode must be one of {sorted(BJ_MODES)}")
        if setup not in self.SETUPS:
            raise ValueError(f"setup must be one of {sorted(self.SETUPS)}")
        h = C.c_void_p()
        check(lib().vtk_bjacobi_create_ex(A.handle, int(bs), self.SETUPS[setup], C.byref(h)), A.ctx.handle)
        self._adopt(h, A, A.values_epoch)
        self.bs = bs
        self.set_mode(mode)

    def refresh(self):
        """Recompute the inverses (and tridiagonal factors) from the operator's current values into
        the storage this preconditioner owns (``vtk_prec_refresh``): the setup it was created
        with and the mode request again.  LinAlgError on a singular block -- the preconditioner
        is then unusable (VtkError, status ERR_STATE) until a later refresh succeeds; ValueError
        when an explicit "tridiag" request can no longer be met (refreshed, applies "inverse")."""
        return _refresh(self)

    @property
    def values_epoch(self) -> int:
        """``A.values_epoch`` of the values the factors were computed from (a lagged
        preconditioner -- older than ``A.values_epoch`` -- is legal)."""
        return self._epoch

    def set_mode(self, mode: str):
        check(lib().vtk_bjacobi_set_mode(self._h, BJ_MODES[mode]), self.A.ctx.handle)

    @property
    def mode(self) -> str:
        """The apply in use: "inverse" or "tridiag"."""
        m = C.c_int()
        check(lib().vtk_bjacobi_get_mode(self._h, C.byref(m), None), self.A.ctx.handle)
        return {1: "inverse", 2: "tridiag"}[m.value]

    @property
    def tridiag_available(self) -> bool:
        t = C.c_int()
        check(lib().vtk_bjacobi_get_mode(self._h, None, C.byref(t)), self.A.ctx.handle)
        return bool(t.value)

    def inverse(self) -> np.ndarray:
        nb = (self.A.n_local + self.bs - 1) // self.bs
        inv = np.empty((nb, self.bs, self.bs))
        check(lib().vtk_bjacobi_inverse(self._h, _np_ptr(inv), _abi.PTR_HOST), self.A.ctx.handle)
        return inv


def block_jacobi(A: CsrOperator, bs: int = 8, mode: str = "auto", setup: str = "exact") -> BlockJacobi:
    return BlockJacobi(A, bs, mode, setup)


class LineJacobi(_Prec):
    """Line-Jacobi preconditioner (line-implicit x-direction solve):
    M = A's diagonal + the couplings between rows R and R +- ``stride`` within segments of
    ``seg`` consecutive line indices R // stride (and within this rank's rows).  SciPy
    statement: ``LinearOperator(matvec=splu(M).solve)``.  ``vtk_linejacobi_create``.

    For the Vlasov operators ``stride`` = 1 (1D), Nv (2D), Ny*Nvx*Nvy (4D): see
    :func:`vlasov_line_stride`.  Choose ``seg`` dividing Nx / world so that M does not depend
    on the number of ranks."""

    def __init__(self, A: CsrOperator, stride: int, seg: int = 25):
        h = C.c_void_p()
        check(lib().vtk_linejacobi_create(A.handle, int(stride), int(seg), C.byref(h)), A.ctx.handle)
        self._adopt(h, A, A.values_epoch)
        self.stride = int(stride)
        self.seg = int(seg)

    def refresh(self):
        """Recompute the Thomas factors from the operator's current values into the storage this
        preconditioner owns and re-run the x-invariance check (``vtk_prec_refresh``): the compact
        apply is dropped or regained accordingly, a ``set_compact(False)`` is kept.  LinAlgError
        on a zero pivot -- unusable (VtkError, status ERR_STATE) until a later refresh succeeds."""
        return _refresh(self)

    @property
    def compact(self) -> bool:
        """Apply forms l and g from the lines' constant x-couplings (reads only m)."""
        u = C.c_int()
        check(lib().vtk_linejacobi_get_compact(self._h, C.byref(u), None), self.A.ctx.handle)
        return bool(u.value)

    @property
    def compact_available(self) -> bool:
        a = C.c_int()
        check(lib().vtk_linejacobi_get_compact(self._h, None, C.byref(a)), self.A.ctx.handle)
        return bool(a.value)

    def set_compact(self, on: bool):
        check(lib().vtk_linejacobi_set_compact(self._h, int(bool(on))), self.A.ctx.handle)

    def factors(self) -> np.ndarray:
        """l | m | g, 3 * n_local doubles (the oracle's orc_line_setup layout)."""
        f = np.empty(3 * self.A.n_local)
        check(lib().vtk_linejacobi_factors(self._h, _np_ptr(f), _abi.PTR_HOST), self.A.ctx.handle)
        return f


def line_jacobi(A: CsrOperator, stride: int, seg: int = 25) -> LineJacobi:
    return LineJacobi(A, stride, seg)


def vlasov_line_stride(params) -> int:
    """Rows between x-neighbours of a Vlasov operator: 1 (1D), Nv (2D), Ny*Nvx*Nvy (4D)."""
    dim = int(params.dim)
    sh = [int(v) for v in params.shape]
    if dim == 1:
        return 1
    if dim == 2:
        return sh[1]
    return sh[1] * sh[2] * sh[3]


def vlasov_line_period(params) -> int:
    """Unknowns of one periodic x-line of a Vlasov operator, Nx: :func:`line_cyclic`'s ``period``
    next to :func:`vlasov_line_stride`'s stride.  (The 4D y-lines: stride Nvx*Nvy, period Ny.)"""
    return int(params.shape[0])


def vlasov_line_directions(params) -> list[int]:
    """The line strides of a Vlasov operator, strongest advection direction first: [1] (1D),
    [Nv, 1] (2D: x, then v), [Ny*Nvx*Nvy, Nvx*Nvy] (4D: x, then y).  The first entry is
    :func:`vlasov_line_stride`; the first two are :func:`line_product`'s directions."""
    dim = int(params.dim)
    sh = [int(v) for v in params.shape]
    if dim == 1:
        return [1]
    if dim == 2:
        return [sh[1], 1]
    return [sh[1] * sh[2] * sh[3], sh[2] * sh[3]]


class LineProduct(_Prec):
    """Two-direction line preconditioner: the approximate-factorisation product
    M = M1 D^-1 M2 = D + X + Y + X D^-1 Y of two :class:`LineJacobi` matrices of ``A``, given as
    ``(stride, seg)`` pairs, with D = A's diagonal.  SciPy statement:
    ``LinearOperator(matvec=lambda r: lu2.solve(D * lu1.solve(r)))`` with ``lu_i = splu(M_i)``.
    ``vtk_lineproduct_create``.

    For the 4D Vlasov operators the directions are x and y: :func:`vlasov_line_directions`."""

    def __init__(self, A: CsrOperator, dir1, dir2):
        (s1, g1), (s2, g2) = dir1, dir2
        h = C.c_void_p()
        check(lib().vtk_lineproduct_create(A.handle, int(s1), int(g1), int(s2), int(g2), C.byref(h)), A.ctx.handle)
        self._adopt(h, A, A.values_epoch)
        self.directions = ((int(s1), int(g1)), (int(s2), int(g2)))

    def refresh(self):
        """Recompute both directions' Thomas factors and D from the operator's current values and
        re-run the constant-coupling check per direction (``vtk_prec_refresh``).  LinAlgError on a
        zero pivot -- unusable (VtkError, status ERR_STATE) until a later refresh succeeds."""
        return _refresh(self)

    def factors(self, which: int) -> np.ndarray:
        """l | m | g of direction ``which`` (0 or 1), 3 * n_local doubles (the oracle's
        orc_line_setup layout)."""
        if which not in (0, 1):
            raise ValueError("LineProduct.factors: which must be 0 or 1")
        f = np.empty(3 * self.A.n_local)
        check(lib().vtk_lineproduct_factors(self._h, int(which), _np_ptr(f), _abi.PTR_HOST), self.A.ctx.handle)
        return f

    def diagonal(self) -> np.ndarray:
        """D: per row the sum of its stored diagonal entries (n_local doubles)."""
        d = np.empty(self.A.n_local)
        check(lib().vtk_lineproduct_factors(self._h, 2, _np_ptr(d), _abi.PTR_HOST), self.A.ctx.handle)
        return d


def line_product(A: CsrOperator, dir1, dir2) -> LineProduct:
    """``line_product(A, (stride1, seg1), (stride2, seg2))``: see :class:`LineProduct`."""
    return LineProduct(A, dir1, dir2)


class LineCyclic(_Prec):
    """Periodic whole-line preconditioner: M = A's diagonal + every coupling
    between rows of one line -- R mod ``stride`` and R // (``stride`` * ``period``) equal -- whose
    line indices (R // stride) mod period differ by +-1 modulo ``period``, the wrap included: one
    cyclic tridiagonal system of ``period`` unknowns per line.  SciPy statement:
    ``LinearOperator(matvec=splu(M).solve)``.  ``vtk_linecyclic_create``.

    ``seg`` is only the partition length of the solver (a recursive Schur complement on
    separators); it does not change M.  Vlasov operators: ``stride`` from
    :func:`vlasov_line_stride`, ``period`` from :func:`vlasov_line_period`.  Every cyclic line
    must lie on one rank (ValueError otherwise) -- unless ``span=True``.

    ``span=True`` (``vtk_linecyclic_create_span``): the lines may span the ranks.
    One block of lines only (``n == stride * period``, ``period`` the global one); every rank owns
    at least 3 whole line indices.  Creation and :meth:`refresh` are then collective -- every rank
    makes the call and every rank raises alike -- and an apply costs one all-gather of
    ``16 * stride`` bytes per rank.  With one rank the same path runs with world 1.  Not accepted
    as the base of :func:`neumann` (ValueError)."""

    def __init__(self, A: CsrOperator, stride: int, period: int, seg: int = 25, span: bool = False):
        h = C.c_void_p()
        create = lib().vtk_linecyclic_create_span if span else lib().vtk_linecyclic_create
        check(create(A.handle, int(stride), int(period), int(seg), C.byref(h)), A.ctx.handle)
        self._adopt(h, A, A.values_epoch)
        self.span = bool(span)
        self.stride = int(stride)
        self.period = int(period)
        self.seg = int(seg)

    def refresh(self):
        """Refactor every level from the operator's current values (``vtk_prec_refresh``).
        LinAlgError on a zero pivot at any level -- unusable (VtkError, status ERR_STATE) until a
        later refresh succeeds."""
        return _refresh(self)

    def info(self) -> dict:
        """``levels`` (the last one is solved by one lane per line), ``unknowns`` per line and
        level, ``compact`` (spikes kept as one table per line; False: stored per row)."""
        o = _abi.LinecInfo()
        check(lib().vtk_linecyclic_info(self._h, C.byref(o)), self.A.ctx.handle)
        return {"levels": int(o.levels), "unknowns": [int(o.unknowns[k]) for k in range(o.levels)],
                "compact": bool(o.compact), "stride": int(o.stride), "period": int(o.period), "seg": int(o.seg)}

    @property
    def span_info(self) -> dict:
        """Of a ``span=True`` preconditioner: ``world``, ``rank``, ``first_line`` (the rank's first
        line index), ``local_period`` (its line indices, P_p), ``period`` and ``spanning`` (True).
        VtkError (status ERR_STATE) for one that does not span."""
        o = _abi.LinecSpanInfo()
        check(lib().vtk_linecyclic_span_info(self._h, C.byref(o)), self.A.ctx.handle)
        return {"world": int(o.world), "rank": int(o.rank), "first_line": int(o.first_line),
                "local_period": int(o.local_period), "period": int(o.period), "spanning": bool(o.spanning)}


def line_cyclic(A: CsrOperator, stride: int, period: int, seg: int = 25, span: bool = False) -> LineCyclic:
    """``line_cyclic(A, stride, period, seg=25, span=False)``: see :class:`LineCyclic`."""
    return LineCyclic(A, stride, period, seg, span)


class Neumann(_Prec):
    """Neumann-series (polynomial) wrapper around any preconditioner ``M`` of ``A``:
    ``degree`` steps of preconditioned Richardson from 0, i.e. the degree-(``degree`` - 1) Neumann
    series of M^-1 A.  More operator work per Krylov vector, fewer Krylov vectors.  SciPy statement::

        def mv(r):
            z = M(r)
            for _ in range(degree - 1):
                z = z + M(r - A @ z)
            return z

        LinearOperator((n, n), matvec=mv)

    ``vtk_neumann_create``.  1 <= ``degree`` <= 8; ``degree`` 1 is ``M`` itself, bit for bit.  With
    block Jacobi, line Jacobi and the line product the result equals that composition of the
    library's own ``A @ x`` and ``M @ x`` bit for bit; with the periodic lines to rounding.

    The wrapper borrows ``M``: it keeps a reference to the Python object, and a wrapper whose base
    was closed raises VtkError (status ERR_STATE) at its next use.  ``M`` must not be a ``Neumann``
    and must belong to ``A`` (ValueError); a ``line_cyclic(..., span=True)`` base is refused as
    well (ValueError).  Whether a degree pays depends on the spectrum of
    M^-1 A: block Jacobi on the Vlasov operators gains at degree 2 and stalls at degree 3; the line
    product gains at every degree.  Nothing selects the wrapper by default."""

    def __init__(self, A: CsrOperator, M, degree: int = 2):
        if not isinstance(M, _PRECS):   # (a Neumann base is the library's VTK_ERR_ARG: ValueError)
            raise TypeError("vtkrylov.neumann: M must be " + _BASE_PRECS_TEXT)
        h = C.c_void_p()
        check(lib().vtk_neumann_create(A.handle, M.handle, int(degree), C.byref(h)), A.ctx.handle)
        self._adopt(h, A, M.values_epoch)
        self.base = M
        self.degree = int(degree)

    def refresh(self):
        """Refresh the base from the operator's current values (``vtk_prec_refresh`` on the wrapper
        refreshes its base; the base's errors pass through)."""
        try:
            return _refresh(self)
        finally:
            self.base._epoch = self._epoch

    @property
    def values_epoch(self) -> int:
        """The base's ``values_epoch``: the wrapper owns no factors."""
        return self.base.values_epoch

    def info(self) -> dict:
        """``degree``, ``base`` (the base's kind), ``fused`` (each correction is one SpMV launch
        with the base in its epilogue: block Jacobi on fused tiles, bs <= 8), ``base_alive``."""
        o = _abi.NeuInfo()
        check(lib().vtk_neumann_info(self._h, C.byref(o)), self.A.ctx.handle)
        return {"degree": int(o.degree), "base": _abi.PREC_KINDS.get(int(o.base_kind)), "fused": bool(o.fused),
                "base_alive": bool(o.base_alive)}


def neumann(A: CsrOperator, M, degree: int = 2) -> Neumann:
    """``neumann(A, M, degree=2)``: see :class:`Neumann`."""
    return Neumann(A, M, degree)


_BASE_PRECS = (BlockJacobi, LineJacobi, LineProduct, LineCyclic)
_BASE_PRECS_TEXT = "a vtkrylov.BlockJacobi, vtkrylov.LineJacobi, vtkrylov.LineProduct or vtkrylov.LineCyclic"
_PRECS = _BASE_PRECS + (Neumann,)
_PRECS_TEXT = ("None, vtkrylov.BlockJacobi, vtkrylov.LineJacobi, vtkrylov.LineProduct, vtkrylov.LineCyclic "
               "or vtkrylov.Neumann")


@dataclass
class SolveStats:
    inner_iters: int
    restarts: int
    presid: float
    rnorm: float
    bnorm: float
    atol_eff: float
    t_solve: float
    bytes_moved: float
    breakdown: int
    orth: int
    band: int = 0   # 1: the line-band DCGS2 step ran


_last_stats: SolveStats | None = None


def last_stats() -> SolveStats | None:
    return _last_stats


@dataclass
class BasisInfo:
    """``vtk_basis_info``: the basis storage set on the context, and what the last :func:`gmres`
    on it used (0 float64, 1 float32) with that solve's basis and workspace bytes."""
    requested: int
    used: int
    basis_bytes: int
    workspace_bytes: int


_last_basis_ctx = None


def last_basis_info() -> BasisInfo | None:
    """:class:`BasisInfo` of the last :func:`gmres` call (None before the first)."""
    return None if _last_basis_ctx is None else _last_basis_ctx.basis_info()


@dataclass
class ArnoldiCapture:
    """One captured restart cycle (``vtk_gmres_captured``; include/vtkrylov.h states which columns
    of ``V`` are final).  ``V``: (restart + 1, n_local), row k = column k of the basis.  ``H``:
    (restart, restart + 1), row c = the rotated column c; ``Hraw`` (DCGS2): (restart + 1,
    restart + 1), row c = the unrotated column c.  ``giv``: (restart, 2) pairs (c, s)."""
    n_local: int
    restart: int
    cycle: int
    cols: int
    final_cols: int
    orth: int
    band: int
    stop_col: int
    breakdown: int
    xup_tag: int
    V: np.ndarray
    x_in: np.ndarray
    H: np.ndarray
    S: np.ndarray
    giv: np.ndarray
    Hraw: np.ndarray | None = None
    committed: np.ndarray | None = None
    nu: float | None = None


def last_arnoldi(ctx: Context | None = None) -> ArnoldiCapture:
    """The restart cycle captured by the last solve under ``ctx.capture_arnoldi`` (VtkError with
    status ERR_STATE when there is none)."""
    ctx = ctx or default_context()
    ai = _abi.ArnoldiInfo()
    check(lib().vtk_gmres_captured(ctx.handle, C.byref(ai)), ctx.handle)
    m, ld, n = ai.restart, ai.ld, ai.n_local

    def rd(what, count, dtype=np.float64):
        a = np.zeros(count, dtype=dtype)
        check(lib().vtk_gmres_captured_read(ctx.handle, what, _np_ptr(a), _abi.PTR_HOST), ctx.handle)
        return a
    out = ArnoldiCapture(
        n_local=n, restart=m, cycle=ai.cycle, cols=ai.cols, final_cols=ai.final_cols, orth=ai.orth, band=ai.band,
        stop_col=ai.stop_col, breakdown=ai.breakdown, xup_tag=ai.xup_tag,
        V=rd(_abi.CAP_V, (m + 1) * ld).reshape(m + 1, ld)[:, :n].copy(), x_in=rd(_abi.CAP_X_IN, n),
        H=rd(_abi.CAP_H, m * (m + 1)).reshape(m, m + 1), S=rd(_abi.CAP_S, m + 1),
        giv=rd(_abi.CAP_GIV, 2 * m).reshape(m, 2))
    if ai.has_hraw:
        out.Hraw = rd(_abi.CAP_HRAW, (m + 1) * (m + 1)).reshape(m + 1, m + 1)
        out.committed = rd(_abi.CAP_COMMITTED, m + 1, np.int32)
        out.nu = float(rd(_abi.CAP_NU, 1)[0])
    return out


def gmres(A, b, x0=None, *, rtol=1e-5, atol=0., restart=None, maxiter=None, M=None,
          callback=None, callback_type=None, orth=None, basis=None):
    """``scipy.sparse.linalg.gmres`` on the GPU (iterative.py:582-841, left-preconditioned
    restarted GMRES: SciPy's control flow, ptol schedule, ``dlartg`` Givens rotations and
    ``info`` convention).  Returns ``(x, info)``.

    Orthogonalisation: the DEFAULT (``orth=None``/``"auto"`` with the context left at auto) is
    DCGS2 -- delayed classical Gram-Schmidt with re-orthogonalisation, one global reduction per
    Arnoldi step -- whenever ``restart <= 32``, else MGS.  DCGS2 builds the same Krylov basis in
    exact arithmetic but not SciPy's floating-point sequence: info matches and the inner
    iteration count may differ by one.  ``orth="mgs"`` runs SciPy's exact
    modified Gram-Schmidt sequence (iterative.py:755-759); ``orth="dcgs2"`` forces DCGS2.

    Basis storage: ``basis=None`` keeps the context's setting (float64 unless
    :meth:`Context.set_basis` changed it); ``basis="float32"`` stores the orthonormal columns in
    float32 and computes in float64 (compressed-basis GMRES, DESIGN.md §3p: about two thirds of
    the workspace, DCGS2 only, no line-band step; results agree with the float64 basis to the
    tolerance, not bit for bit); ``basis="float64"`` forces the full basis.  Any other value
    raises ValueError.  :func:`last_basis_info` reports what the solve used.

    ``A``: a :class:`CsrOperator` or any SciPy sparse matrix (uploaded).  ``M``: None, a
    :class:`BlockJacobi`, a :class:`LineJacobi`, a :class:`LineProduct`, a :class:`LineCyclic` or a :class:`Neumann` wrapper built on ``A``; any other preconditioner raises TypeError (no CPU
    fallback).  ``callback`` is not supported (the Arnoldi loop never returns to the host).
    ``restart``/``maxiter``: None = SciPy's defaults (20 / 10 n); explicit values must be
    positive integers (ValueError otherwise).
    """
    global _last_stats, _last_basis_ctx
    if basis is not None and (not isinstance(basis, str) or basis not in _abi.BASIS):
        raise ValueError(f"vtkrylov.gmres: basis must be None, 'float64' or 'float32', got {basis!r}")
    if callback is not None:
        raise NotImplementedError("vtkrylov.gmres: callbacks would force a host round trip per "
                                  "Arnoldi step and are not supported")
    if M is not None and not isinstance(M, _PRECS):
        raise TypeError("vtkrylov.gmres: M must be " + _PRECS_TEXT)
    if not isinstance(A, CsrOperator):
        A = csr_matrix(A)
    if atol == "legacy" or atol is None or atol < 0:
        raise ValueError(f"'scipy.sparse.linalg.gmres' called with invalid `atol`={atol}; "
                         "if set, `atol` must be a real, non-negative number.")
    for name, v in (("restart", restart), ("maxiter", maxiter)):
        if v is not None and (int(v) != v or int(v) <= 0):
            raise ValueError(f"vtkrylov.gmres: {name} must be a positive integer or None, got {v!r}")
    n = A.n_local
    vb = _Vec(b, n)
    if x0 is None:
        if vb.kind == _abi.PTR_DEVICE:
            import torch
            x = torch.zeros_like(vb.obj)
        else:
            x = np.zeros(n)
    else:
        if vb.kind == _abi.PTR_DEVICE:
            x = x0.clone()
        else:
            x = np.array(x0, dtype=np.float64, copy=True).reshape(-1)
    vx = _Vec(x, n, writable=True)
    x = vx.obj
    info = C.c_int()
    st = _abi.Stats()
    prev = None
    if orth is not None:
        prev = A.ctx.orth
        A.ctx.set_orth(_abi.ORTH[orth])
    prev_basis = None
    if basis is not None:
        prev_basis = A.ctx.basis
        A.ctx.set_basis(_abi.BASIS[basis])
    _last_basis_ctx = A.ctx
    try:
        check(lib().vtk_gmres(A.handle, None if M is None else M.handle, vb.ptr, vx.ptr,
                              float(rtol), float(atol), 0 if restart is None else int(restart),
                              0 if maxiter is None else int(maxiter), vb.kind, C.byref(info),
                              C.byref(st)), A.ctx.handle)
    finally:
        if prev is not None:
            A.ctx.set_orth(prev)
        if prev_basis is not None:
            A.ctx.set_basis(prev_basis)
    _last_stats = SolveStats(**st.as_dict())
    return x, info.value


@dataclass
class BicgstabStats:
    iterations: int    # v = A M p products computed
    rnorm: float       # true residual ||b - A x|| of the returned x
    bnorm: float
    atol_eff: float
    t_solve: float
    bytes_moved: float
    half_step: int     # 1: left through the ||s|| test (SciPy's callback count is iterations - half_step)


_last_bicgstab_stats: BicgstabStats | None = None


def last_bicgstab_stats() -> BicgstabStats | None:
    return _last_bicgstab_stats


def bicgstab(A, b, x0=None, *, rtol=1e-5, atol=0., maxiter=None, M=None, callback=None):
    """``scipy.sparse.linalg.bicgstab`` on the GPU (iterative.py, ``bicgstab``: right-preconditioned,
    SciPy's control flow, breakdown tests and ``info`` convention: 0 converged, -10 / -11 a
    breakdown, else ``maxiter``).  Returns ``(x, info)``.

    Seven work vectors whatever the problem, no restart parameter.  The reductions are summed in
    the device's fixed order, not NumPy's: the iterate is deterministic from run to run and agrees
    with SciPy's to the tolerance, not bit for bit, and the iteration count may differ by a few
    (INTEGRATION.md).

    Across ranks (a context with a communicator): ``b``, ``x0`` and the returned ``x`` are this
    rank's rows, as for :func:`gmres`; every rank calls with the same tolerances and ``maxiter``.
    The sums of an iteration are all-reduced (four small collectives per iteration), so ``info``
    and every field of :func:`last_bicgstab_stats` but the timing are the same on every rank.  A
    rank whose launch fails mid-solve raises its own error and the others raise ERR_PEER at the
    same point; the communicator stays usable.

    ``A``: a :class:`CsrOperator` or any SciPy sparse matrix (uploaded).  ``M``: None, a
    :class:`BlockJacobi`, a :class:`LineJacobi` or a :class:`LineProduct` built on ``A``; any other preconditioner raises
    TypeError (no CPU fallback).  ``callback`` is not supported (the loop never returns to the
    host).  ``maxiter``: None = SciPy's default (10 n); an explicit value must be a positive integer.
    """
    global _last_bicgstab_stats
    if callback is not None:
        raise NotImplementedError("vtkrylov.bicgstab: callbacks would force a host round trip per "
                                  "iteration and are not supported")
    if M is not None and not isinstance(M, _PRECS):
        raise TypeError("vtkrylov.bicgstab: M must be " + _PRECS_TEXT)
    if atol == "legacy" or atol is None or atol < 0:
        raise ValueError(f"'scipy.sparse.linalg.bicgstab' called with invalid `atol`={atol}; "
                         "if set, `atol` must be a real, non-negative number.")
    if maxiter is not None and (int(maxiter) != maxiter or int(maxiter) <= 0):
        raise ValueError(f"vtkrylov.bicgstab: maxiter must be a positive integer or None, got {maxiter!r}")
    if not isinstance(A, CsrOperator):
        A = csr_matrix(A)
    n = A.n_local
    vb = _Vec(b, n)
    if x0 is None:
        if vb.kind == _abi.PTR_DEVICE:
            import torch
            x = torch.zeros_like(vb.obj)
        else:
            x = np.zeros(n)
    else:
        if vb.kind == _abi.PTR_DEVICE:
            x = x0.clone()
        else:
            x = np.array(x0, dtype=np.float64, copy=True).reshape(-1)
    vx = _Vec(x, n, writable=True)
    x = vx.obj
    info = C.c_int()
    st = _abi.BicgstabStats()
    check(lib().vtk_bicgstab(A.handle, None if M is None else M.handle, vb.ptr, vx.ptr, float(rtol), float(atol),
                             0 if maxiter is None else int(maxiter), vb.kind, C.byref(info), C.byref(st)),
          A.ctx.handle)
    _last_bicgstab_stats = BicgstabStats(**st.as_dict())
    return x, info.value


def rhs_splitmix(n: int, seed: int = 0x5EED, r0: int = 0, r1: int | None = None) -> np.ndarray:
    r1 = n if r1 is None else r1
    b = np.empty(r1 - r0)
    check(lib().vtk_rhs_splitmix(seed, r0, r1, _np_ptr(b)))
    return b


def vlasov_generate_host(params: VlasovParams, r0: int = 0, r1: int | None = None):
    """Host assembly of rows [r0, r1) (the same entry code the device generator runs)."""
    n, nnz = C.c_int64(), C.c_int64()
    check(lib().vtk_vlasov_size(C.byref(params), C.byref(n), C.byref(nnz)))
    r1 = n.value if r1 is None else r1
    per = {1: 3, 2: 5, 4: 9}[params.dim]
    cap = max(1, (r1 - r0) * per)
    ip = np.empty(r1 - r0 + 1, np.int32)
    ix = np.empty(cap, np.int32)
    d = np.empty(cap, np.float32 if params.fp32 else np.float64)
    check(lib().vtk_vlasov_generate(C.byref(params), r0, r1, _np_ptr(ip), _np_ptr(ix), _np_ptr(d)))
    k = int(ip[-1])
    return ip, ix[:k].copy(), d[:k].copy()


def partition_rows(n: int, world: int, align: int = 1, indptr=None) -> np.ndarray:
    offs = np.empty(world + 1, np.int64)
    ip = None if indptr is None else np.ascontiguousarray(indptr, np.int32)
    check(lib().vtk_partition_rows(n, None if ip is None else _np_ptr(ip), world, align, _np_ptr(offs)))
    return offs


def halo_plan(n_global: int, offsets, rank: int, indices):
    """(local_indices, halo_cols, halo_count_per_rank) of one rank's row block."""
    offs = np.ascontiguousarray(offsets, np.int64)
    world = offs.shape[0] - 1
    idx = np.ascontiguousarray(indices, np.int32)
    nh = C.c_int64()
    check(lib().vtk_halo_plan(n_global, _np_ptr(offs), world, rank, idx.shape[0], _np_ptr(idx),
                              None, C.byref(nh), None, None))
    loc = np.empty(idx.shape[0], np.int32)
    cols = np.empty(max(nh.value, 1), np.int64)
    cnt = np.empty(world, np.int64)
    check(lib().vtk_halo_plan(n_global, _np_ptr(offs), world, rank, idx.shape[0], _np_ptr(idx),
                              _np_ptr(loc), C.byref(nh), _np_ptr(cols), _np_ptr(cnt)))
    return loc, cols[:nh.value], cnt
