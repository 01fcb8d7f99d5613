"""The value-update entry points on the CPU: include/vtkrylov.h declares them, libvtkrylov.so
exports them, vtkrylov._abi.PROTOTYPES binds them, the ABI version stays 6, and NULL handles are
refused with VTK_ERR_ARG before any device is touched."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "vtkrylov.h")
NEW = ["vtk_csr_update_values", "vtk_csr_update_vlasov", "vtk_csr_values_epoch", "vtk_prec_refresh"]


def test_header_declares_library_exports_and_binding_has_them(vk_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = ctypes.CDLL(vk_lib._abi.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} not declared in vtkrylov.h"
        assert hasattr(L, name), f"{name} not exported"
        assert name in vk_lib._abi.PROTOTYPES, f"{name} not in _abi.PROTOTYPES"
        assert vk_lib._abi.PROTOTYPES[name][0] is ctypes.c_int


def test_abi_version_unchanged(vk_lib):
    assert vk_lib._abi.lib().vtk_abi_version() == vk_lib._abi.ABI_VERSION == 6
    assert re.search(r"#define\s+VTK_ABI_VERSION\s+6\b", open(HEADER).read())


def test_null_handles_are_refused_without_a_device(vk_lib):
    L = vk_lib._abi.lib()
    e = ctypes.c_int64(-7)
    d = (ctypes.c_double * 4)()
    p = vk_lib.vlasov_params(2, (64, 32))
    assert L.vtk_csr_update_values(None, d, vk_lib._abi.PTR_HOST) == vk_lib._abi.ERR_ARG
    assert "vtk_csr_update_values" in vk_lib._abi.last_error()
    assert L.vtk_csr_update_vlasov(None, ctypes.byref(p)) == vk_lib._abi.ERR_ARG
    assert "vtk_csr_update_vlasov" in vk_lib._abi.last_error()
    assert L.vtk_csr_values_epoch(None, ctypes.byref(e)) == vk_lib._abi.ERR_ARG
    assert e.value == -7
    assert L.vtk_prec_refresh(None, ctypes.byref(e)) == vk_lib._abi.ERR_ARG
    assert L.vtk_prec_refresh(None, None) == vk_lib._abi.ERR_ARG
    assert "vtk_prec_refresh" in vk_lib._abi.last_error()
    assert e.value == -7


def test_python_surface(vk_lib):
    """The Python layer exposes the update path on the classes users hold."""
    for name in ("update_values", "update_vlasov", "values_epoch"):
        assert hasattr(vk_lib.CsrOperator, name), name
    for cls in (vk_lib.BlockJacobi, vk_lib.LineJacobi):
        assert callable(getattr(cls, "refresh")) and isinstance(cls.values_epoch, property)
