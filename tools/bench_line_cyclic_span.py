"""The cost of the rank level of the cyclic lines on one GPU, in one process.

After one warm-up solve of each, `--reps` rounds alternate vtkrylov.gmres with the plain
line_cyclic(A, Nv, Nx, 25) and with line_cyclic(A, Nv, Nx, 25, span=True) -- the spike path with
world 1: the same chunk solve, plus V_p / W_p in the last sweep, the edge kernel, a device copy in
place of the all-gather, and the interface solve -- on the right-hand side rhs_splitmix as a device
tensor, x0 = 0, rtol 1e-8, restart 20.  Reported per variant: the median of the library's own
t_solve, the inner iterations, and the true residual ||b - A x|| / ||b|| recomputed with the device
SpMV.  Then, in a run of its own, one more solve of each under the per-kernel event profile:
algorithmic bytes / event time per kernel class, and for the phases of either apply their bytes,
microseconds and fraction of 8 TB/s.  The comparison object is the plain kind.  No run across
several GPUs is made here: the figure is what the rank level costs where nothing is gained from it.

    python tools/bench_line_cyclic_span.py --config C1|C2|C3 [--reps 3] [--seg 25] [--serial 64]

Prints one JSON line and appends it to profiles/line_cyclic_span_bench.jsonl.  Reads nothing outside
the repository.  Needs the GPU: no fallback.  One process per configuration."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vt-precondition_amd")]

HBM_BYTES_PER_S = 8.0e12
PHASES = ("linec_sweep", "linec_reduced", "linec_correct", "linec_span", "linec_correct_span")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C1", "C2", "C3", "S2"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--seg", type=int, default=25, help="segment length of both preconditioners")
    ap.add_argument("--serial", type=int, default=64, help="tuning linec_serial at creation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_cyclic_span_bench.jsonl"))
    a = ap.parse_args()
    import torch   # first: one HIP runtime for torch and the library

    import vtkrylov as vk
    from oracle import twin
    vk._abi.check_build_id()
    if vk.device_count() < 1:
        raise SystemExit("bench_line_cyclic_span: no HIP device (measurements need the GPU)")
    ctx = vk.default_context(0)
    p = twin.CONFIGS[a.config]
    prm = vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)
    A = vk.vlasov_operator(prm, ctx=ctx)
    stride, period = vk.vlasov_line_stride(prm), vk.vlasov_line_period(prm)
    with ctx.tuning(linec_serial=a.serial):
        prec = {"plain": vk.line_cyclic(A, stride, period, a.seg), "span": vk.line_cyclic(A, stride, period, a.seg, span=True)}
    n = A.n_local
    b = torch.from_numpy(vk.rhs_splitmix(n)).to(torch.device("cuda", 0))
    bnorm = float(torch.linalg.vector_norm(b))

    def solve(k):
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
    out = {"tool": "bench_line_cyclic_span", "config": a.config, "n": n, "nnz": A.nnz, "rtol": a.rtol, "restart": 20,
           "reps": a.reps, "layout": A.layout, "seg": a.seg, "stride": stride, "period": period,
           "linec": prec["span"].info(), "span_info": prec["span"].span_info, "ranks_measured": 1}
    for k, rr in res.items():
        last = rr[-1]
        out[k] = {"ms_median": round(statistics.median(r["t"] for r in rr) * 1e3, 4),
                  "ms": [round(r["t"] * 1e3, 4) for r in rr], **{q: last[q] for q in last if q != "t"}}
    out["span_over_plain"] = {"ms": round(out["span"]["ms_median"] / out["plain"]["ms_median"], 4),
                              "iterations": round(out["span"]["iterations"] / out["plain"]["iterations"], 4)}
    prof, phases = {}, {}
    for k in prec:   # a run of its own: the events serialise the launches
        ctx.profile(True)
        solve(k)
        pr = ctx.profile_read()
        ctx.profile(False)
        prof[k] = {c: {"launches": v["launches"], "avg_us": round(v["avg_us"], 2), "gbs": round(v["gbs"], 1)}
                   for c, v in sorted(pr.items(), key=lambda kv: -kv[1]["seconds"])}
        phases[k] = {c: {"avg_us": round(pr[c]["avg_us"], 2), "bytes": round(pr[c]["bytes"] / pr[c]["launches"]),
                         "fraction_of_8TBs": round(pr[c]["bytes"] / pr[c]["seconds"] / HBM_BYTES_PER_S, 4)}
                     for c in PHASES if c in pr}
    out["phases"] = phases
    out["kernels"] = prof
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(out) + "\n")
    for o in (*prec.values(), A):
        o.close()


if __name__ == "__main__":
    main()
