"""BiCGStab against restarted GMRES on one operator, in one process.

After one warm-up solve of each, `--reps` rounds alternate vtkrylov.bicgstab (tuning bcg_fuse 1),
vtkrylov.bicgstab with bcg_fuse 0 (block Jacobi only: the separate preconditioner apply) and
vtkrylov.gmres, the right-hand side rhs_splitmix as a device tensor, x0 = 0, rtol 1e-8; the
reported times are the medians of the library's own t_solve.  Then one more solve of each under
the per-kernel event profile: algorithmic bytes / event time per kernel class.

    python tools/bench_bicgstab.py --config C1|C3|C4 --prec bj|line|none [--reps 3] [--rtol 1e-8]

--comm-solo: the cost of the rank path on one GPU.  The rounds alternate vtkrylov.bicgstab on the
plain context and on a second context with a one-rank RCCL communicator (tuning comm_solo: the
distributed code path -- k_bcg_reduce and four all-reduces per iteration), each with its own
operator and preconditioner; GMRES is left out.  The record then carries the microseconds per
iteration of the reduce + all-reduce classes (write it to profiles/bicgstab_ranks.jsonl with --out).

Prints one JSON line and appends it to profiles/bicgstab_bench.jsonl.  Reads nothing outside the
repository.  Needs the GPU: no fallback.  One process per configuration."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vt-precondition_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C1", "C2", "C3", "C4"])
    ap.add_argument("--prec", default="bj", choices=["bj", "line", "none"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=2000, help="BiCGStab iteration cap")
    ap.add_argument("--comm-solo", action="store_true", help="alternate the plain context with a one-rank RCCL one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicgstab_bench.jsonl"))
    a = ap.parse_args()
    import torch   # first: one HIP runtime for torch and the library

    import vtkrylov as vk
    from oracle import twin
    vk._abi.check_build_id()
    if vk.device_count() < 1:
        raise SystemExit("bench_bicgstab: no HIP device (measurements need the GPU)")
    ctx = vk.default_context(0)
    p = twin.CONFIGS[a.config]
    prm = vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)
    A = vk.vlasov_operator(prm, ctx=ctx)
    M = None
    if a.prec == "bj":
        M = vk.block_jacobi(A, 8)
    elif a.prec == "line":
        M = vk.line_jacobi(A, vk.vlasov_line_stride(prm), 25)
    n = A.n_local
    b = torch.from_numpy(vk.rhs_splitmix(n)).to(torch.device("cuda", 0))

    def bicg(fuse):
        with ctx.tuning(bcg_fuse=fuse):
            x, info = vk.bicgstab(A, b, rtol=a.rtol, M=M, maxiter=a.maxiter)
        st = vk.last_bicgstab_stats()
        return {"info": info, "iterations": st.iterations, "half_step": st.half_step, "t": st.t_solve,
                "rnorm_over_atol": st.rnorm / st.atol_eff, "bytes_moved": st.bytes_moved}

    def gm():
        x, info = vk.gmres(A, b, rtol=a.rtol, M=M)
        st = vk.last_stats()
        return {"info": info, "iterations": st.inner_iters, "restarts": st.restarts, "t": st.t_solve,
                "rnorm_over_atol": st.rnorm / st.atol_eff, "band": st.band, "bytes_moved": st.bytes_moved}

    runs = {"bicgstab": lambda: bicg(1), "gmres": gm}
    if a.prec == "bj":
        runs["bicgstab_unfused"] = lambda: bicg(0)
    solo = []
    if a.comm_solo:
        os.environ["VTK_COMM_SOLO"] = "1"
        try:
            sctx = vk.Context(0)
            sctx.comm_init(0, 1, vk.Context.unique_id())
        finally:
            del os.environ["VTK_COMM_SOLO"]
        As = vk.vlasov_operator(prm, ctx=sctx)
        Ms = None
        if a.prec == "bj":
            Ms = vk.block_jacobi(As, 8)
        elif a.prec == "line":
            Ms = vk.line_jacobi(As, vk.vlasov_line_stride(prm), 25)
        solo = [Ms, As]

        def bicg_solo():
            x, info = vk.bicgstab(As, b, rtol=a.rtol, M=Ms, maxiter=a.maxiter)
            st = vk.last_bicgstab_stats()
            return {"info": info, "iterations": st.iterations, "half_step": st.half_step, "t": st.t_solve,
                    "rnorm_over_atol": st.rnorm / st.atol_eff, "bytes_moved": st.bytes_moved}
        runs = {"bicgstab": lambda: bicg(1), "bicgstab_solo": bicg_solo}
    for fn in runs.values():   # warm-up: code objects, workspace
        fn()
    res = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            res[k].append(fn())
    out = {"tool": "bench_bicgstab", "config": a.config, "prec": a.prec, "n": n, "nnz": A.nnz, "fp32": bool(p.fp32),
           "rtol": a.rtol, "reps": a.reps, "layout": A.layout,
           "work_vectors_bytes": {"bicgstab": 7 * 8 * n, "gmres_restart20": 24 * 8 * n}}
    for k, rr in res.items():
        last = rr[-1]
        out[k] = {"ms_median": round(statistics.median(r["t"] for r in rr) * 1e3, 4),
                  "ms": [round(r["t"] * 1e3, 4) for r in rr], **{q: last[q] for q in last if q != "t"}}
    prof = {}
    for k, fn in runs.items():
        pctx = sctx if k == "bicgstab_solo" else ctx
        pctx.profile(True)
        fn()
        pr = pctx.profile_read()
        pctx.profile(False)
        if k == "bicgstab_solo":   # the rank path's own classes, per iteration that counts
            us = sum(pr[c]["seconds"] for c in ("bcg_reduce", "allreduce") if c in pr) * 1e6
            out[k]["reduce_allreduce_us_per_iteration"] = round(us / max(1, out[k]["iterations"]), 2)
        prof[k] = {c: {"launches": v["launches"], "avg_us": round(v["avg_us"], 2), "gbs": round(v["gbs"], 1)}
                   for c, v in sorted(pr.items(), key=lambda kv: -kv[1]["seconds"])}
    out["kernels"] = prof
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(out) + "\n")
    for o in (*solo, M, A):
        if o is not None:
            o.close()


if __name__ == "__main__":
    main()
