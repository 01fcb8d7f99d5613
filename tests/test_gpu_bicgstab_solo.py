"""vtkrylov.bicgstab over the production RCCL transport on the one-GPU box: a one-rank RCCL
communicator (VTK_COMM_SOLO=1, as tests/test_gpu_rccl_solo.py) takes the solve through the rank
path -- k_bcg_reduce, ncclAllReduce of the small records, the device-state end of the loop -- and the
results must meet the one-rank bars of tests/test_gpu_bicgstab.py.  (Several ranks on one GPU go
through the host-staged transport in tests/test_gpu_bicgstab_ranks.py.)"""
import numpy as np
import pytest

from oracle import twin
from test_gpu_bicgstab import MAXIT, cfg, device_prec, gen, ref, within_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solo(vk_lib):
    import os
    os.environ["VTK_COMM_SOLO"] = "1"
    try:
        ctx = vk_lib.Context(0)
        ctx.comm_init(0, 1, vk_lib.Context.unique_id())
    finally:
        del os.environ["VTK_COMM_SOLO"]
    return ctx


@pytest.mark.parametrize("name,kind", [("C1", "bj8"), ("C1", "line"), ("S4", "bj8")])
def test_rccl_solo_bicgstab(vk_lib, solo, name, kind):
    vk = vk_lib
    p = cfg(name)
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=solo)
    M = device_prec(vk, A, name, kind)
    b = twin.rhs(p.n)
    solo.profile(True)
    x, info = vk.bicgstab(A, b, rtol=1e-8, M=M, maxiter=MAXIT)
    prof = solo.profile_read()
    solo.profile(False)
    st = vk.last_bicgstab_stats()
    r = ref(name, kind, 1e-8)
    within_bars(x, info, st, r, gen(name), b, 1e-8)
    if kind == "line":   # sharp on one rank (test_line_cases_are_sharp): equal count and exit, 1e-9
        assert (st.iterations, st.half_step) == (r[2], r[3])
        assert np.linalg.norm(x - r[0]) / np.linalg.norm(r[0]) <= 1e-9
    # the rank path ran: the small records were summed and all-reduced over RCCL
    assert "allreduce" in prof and prof["allreduce"]["launches"] > 0, sorted(prof)
    assert "bcg_reduce" in prof and prof["bcg_reduce"]["launches"] > 0, sorted(prof)
    M.close()
    A.close()
