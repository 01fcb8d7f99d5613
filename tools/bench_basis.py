#!/usr/bin/env python3
"""float64 against float32 Krylov basis (vtk_gmres_set_basis), measured in one process.

Per case the two kinds of solve alternate (f64, f32, f64, f32, ...) on one operator and one context;
the medians of ``--reps`` solves each are reported, with the inner iterations, the true residual
||b - A x|| recomputed with vtk_spmv, the solver's workspace bytes and -- from one more, profiled solve
per kind (the kernel profile costs a few microseconds per launch, so it is kept out of the timings) --
the achieved fraction of ``--peak`` GB/s of the two basis passes (cb_dots / cb_update against dc_dots /
dc_update; the band step where it runs).  One JSON line per case goes to ``--out``.

Cases: C4 / BJ(8), C4 / line_product, C3 / line_jacobi, C3 / BJ(8) (the float64 solve takes the
line-band step there, the float32 one the compressed split step), C1 / BJ(8).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vt-precondition_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [("C4", "bj8"), ("C4", "line_product"), ("C3", "line_jacobi"), ("C3", "bj8"), ("C1", "bj8")]
SHAPES = {"C1": (2, (1250, 800), False), "C3": (2, (25000, 800), False), "C4": (4, (200, 125, 50, 40), True),
          "S2": (2, (64, 32), False), "S4F": (4, (6, 5, 8, 8), True)}
PASSES = ("cb_dots", "cb_update", "dc_dots", "dc_update", "band_step", "cb_xupdate", "xupdate", "cb_scale0", "scale0")


def preconditioner(vk, A, params, kind, seg):
    if kind == "bj8":
        return vk.block_jacobi(A, 8)
    if kind == "line_jacobi":
        return vk.line_jacobi(A, vk.vlasov_line_stride(params), seg)
    if kind == "line_product":
        d = vk.vlasov_line_directions(params)
        return vk.line_product(A, (d[0], seg), (d[1], seg))
    raise ValueError(kind)


def run_case(vk, torch, ctx, config, kind, a):
    dim, shape, fp32 = SHAPES[config]
    params = vk.vlasov_params(dim, shape, fp32=fp32)
    A = vk.vlasov_operator(params, ctx=ctx)
    M = preconditioner(vk, A, params, kind, a.seg)
    dev = torch.device("cuda", 0)
    b = torch.from_numpy(vk.rhs_splitmix(A.n_global)).to(dev)
    bn = float(torch.linalg.vector_norm(b))
    rec = {"config": config, "preconditioner": kind, "rows": A.n_global, "restart": a.restart, "rtol": a.rtol,
           "reps": a.reps, "peak_gbs": a.peak}
    ms = {"float64": [], "float32": []}
    try:
        for basis in ("float64", "float32"):                     # warm-up, and the workspace grown once
            vk.gmres(A, b, rtol=a.rtol, restart=a.restart, M=M, basis=basis)
        for _ in range(a.reps):
            for basis in ("float64", "float32"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                x, info = vk.gmres(A, b, rtol=a.rtol, restart=a.restart, M=M, basis=basis)
                ms[basis].append((time.perf_counter() - t) * 1e3)
                st, bi = vk.last_stats(), vk.last_basis_info()
                r = float(torch.linalg.vector_norm(b - (A @ x)))
                rec[basis] = {"info": info, "inner_iters": st.inner_iters, "cycles": st.restarts, "band": st.band,
                              "used": bi.used, "true_resid": r, "true_resid_rel": r / bn, "atol_eff": st.atol_eff,
                              "workspace_bytes": bi.workspace_bytes, "basis_bytes": bi.basis_bytes,
                              "bytes_moved": st.bytes_moved}
                del x
        for basis in ("float64", "float32"):
            ctx.profile(True)
            vk.gmres(A, b, rtol=a.rtol, restart=a.restart, M=M, basis=basis)
            prof = ctx.profile_read()
            ctx.profile(False)
            rec[basis]["ms_per_solve"] = statistics.median(ms[basis])
            rec[basis]["ms_all"] = [round(v, 3) for v in ms[basis]]
            rec[basis]["us_per_iter"] = statistics.median(ms[basis]) * 1e3 / max(rec[basis]["inner_iters"], 1)
            rec[basis]["passes"] = {k: {"launches": e["launches"], "avg_us": e["avg_us"], "gbs": e["gbs"],
                                        "frac_peak": e["gbs"] / a.peak} for k, e in prof.items() if k in PASSES}
        rec["speedup"] = rec["float64"]["ms_per_solve"] / rec["float32"]["ms_per_solve"]
        rec["workspace_ratio"] = rec["float32"]["workspace_bytes"] / rec["float64"]["workspace_bytes"]
    finally:
        M.close()
        A.close()
        del b
        torch.cuda.empty_cache()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basis_f32_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=3, help="timed solves of each kind per case (>= 3)")
    ap.add_argument("--restart", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--seg", type=int, default=25, help="line segment length of the line preconditioners")
    ap.add_argument("--peak", type=float, default=8000.0, help="HBM peak in GB/s the fractions refer to")
    ap.add_argument("--cases", default=",".join(f"{c}/{k}" for c, k in CASES))
    a = ap.parse_args(argv)
    if a.reps < 3:
        ap.error("--reps must be at least 3")
    import torch

    import vtkrylov as vk
    vk._abi.check_build_id()
    ctx = vk.default_context(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for case in a.cases.split(","):
            config, kind = case.split("/")
            rec = run_case(vk, torch, ctx, config, kind, a)
            f.write(json.dumps(rec) + "\n")
            f.flush()
            d, s = rec["float64"], rec["float32"]
            print(f"{case}: f64 {d['ms_per_solve']:.2f} ms {d['inner_iters']} it (band {d['band']}) | "
                  f"f32 {s['ms_per_solve']:.2f} ms {s['inner_iters']} it | x{rec['speedup']:.3f} | workspace "
                  f"{d['workspace_bytes'] / 1e9:.2f} -> {s['workspace_bytes'] / 1e9:.2f} GB", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
