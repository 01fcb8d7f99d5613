"""The two-direction line preconditioner against the x-line preconditioner, in one process
(DESIGN.md §3l).

After one warm-up solve of each, `--reps` rounds alternate vtkrylov.gmres with
line_jacobi(A, stride_x, 25) and with line_product(A, (stride_x, 25), (stride_2, 25)) -- stride_2
the second entry of vlasov_line_directions: y on the 4D operators, v on the 2D ones -- on the
right-hand side rhs_splitmix as a device tensor, x0 = 0, rtol 1e-8, restart 20.  Reported per
variant: the median of the library's own t_solve, the inner iterations, and the true residual
||b - A x|| / ||b|| recomputed with the device SpMV.  Then one more solve of each under the
per-kernel event profile: algorithmic bytes / event time per kernel class, and the second sweep's
microseconds and fraction of 8 TB/s.

    python tools/bench_line_product.py --config C4|C1|C3 [--reps 3] [--line2-dc 1|0]

Prints one JSON line and appends it to profiles/line_product_bench.jsonl.  Reads nothing outside
the repository.  Needs the GPU: no fallback.  One process per configuration."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vt-precondition_amd")]

SEG = 25
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4", choices=["C1", "C2", "C3", "C4"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--line2-dc", type=int, default=1, choices=[0, 1], help="tuning line2_dc of the product's solves")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_product_bench.jsonl"))
    a = ap.parse_args()
    import torch   # first: one HIP runtime for torch and the library

    import vtkrylov as vk
    from oracle import twin
    vk._abi.check_build_id()
    if vk.device_count() < 1:
        raise SystemExit("bench_line_product: no HIP device (measurements need the GPU)")
    ctx = vk.default_context(0)
    p = twin.CONFIGS[a.config]
    prm = vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)
    A = vk.vlasov_operator(prm, ctx=ctx)
    s1, s2 = vk.vlasov_line_directions(prm)[:2]
    prec = {"line_x": vk.line_jacobi(A, s1, SEG), "product": vk.line_product(A, (s1, SEG), (s2, SEG))}
    n = A.n_local
    b = torch.from_numpy(vk.rhs_splitmix(n)).to(torch.device("cuda", 0))
    bnorm = float(torch.linalg.vector_norm(b))

    def solve(k):
        with ctx.tuning(line2_dc=a.line2_dc):
            x, info = vk.gmres(A, b, rtol=a.rtol, restart=20, M=prec[k])
        st = vk.last_stats()
        res = float(torch.linalg.vector_norm(b - A.matvec(x))) / bnorm
        return {"info": info, "iterations": st.inner_iters, "restarts": st.restarts, "t": st.t_solve,
                "true_resid_over_bnorm": res, "orth": st.orth, "bytes_moved": st.bytes_moved}

    for k in prec:   # warm-up: code objects, workspace
        solve(k)
    res = {k: [] for k in prec}
    for _ in range(a.reps):
        for k in prec:
            res[k].append(solve(k))
    out = {"tool": "bench_line_product", "config": a.config, "n": n, "nnz": A.nnz, "fp32": bool(p.fp32),
           "rtol": a.rtol, "restart": 20, "reps": a.reps, "layout": A.layout, "seg": SEG, "strides": [s1, s2],
           "line2_dc": a.line2_dc}
    for k, rr in res.items():
        last = rr[-1]
        out[k] = {"ms_median": round(statistics.median(r["t"] for r in rr) * 1e3, 4),
                  "ms": [round(r["t"] * 1e3, 4) for r in rr], **{q: last[q] for q in last if q != "t"}}
    out["product_over_line_x"] = {"ms": round(out["product"]["ms_median"] / out["line_x"]["ms_median"], 4),
                                  "iterations": round(out["product"]["iterations"] / out["line_x"]["iterations"], 4)}
    prof = {}
    for k in prec:
        ctx.profile(True)
        solve(k)
        pr = ctx.profile_read()
        ctx.profile(False)
        prof[k] = {c: {"launches": v["launches"], "avg_us": round(v["avg_us"], 2), "gbs": round(v["gbs"], 1)}
                   for c, v in sorted(pr.items(), key=lambda kv: -kv[1]["seconds"])}
        if k == "product":   # the second sweep (with the step's dots when line2_dc is 1)
            cls = "line2_dc" if a.line2_dc else "line2_sweep"
            if cls in pr:
                out["second_sweep"] = {"class": cls, "avg_us": round(pr[cls]["avg_us"], 2), "gbs": round(pr[cls]["gbs"], 1),
                                       "fraction_of_8TBs": round(pr[cls]["bytes"] / pr[cls]["seconds"] / HBM_BYTES_PER_S, 4)}
    out["kernels"] = prof
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(out) + "\n")
    for o in (*prec.values(), A):
        o.close()


if __name__ == "__main__":
    main()
