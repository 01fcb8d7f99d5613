"""The Neumann-series wrapper against its base preconditioner, in one process.

Degree 1 is the base preconditioner ITSELF on its own fastest path -- for block Jacobi (8) on the 2D
operators that is the line-band DCGS2 step, which a wrapped M cannot take -- so it is the parent
library's figure for that base, measured in the same process.  Degrees 2, 3 and 4 are
vtkrylov.neumann(A, M, degree).  After one warm-up solve of each variant, `--reps` rounds alternate
them: vtkrylov.gmres on the right-hand side rhs_splitmix as a device tensor, x0 = 0, rtol 1e-8,
restart 20, at most `--maxiter` restart cycles (a degree that has not converged by then -- block
Jacobi beyond degree 2, DESIGN.md §3n -- is reported with its info and left out of the timed rounds).
Reported per variant: the median of the library's own t_solve, the inner iterations, and the true
residual ||b - A x|| / ||b|| recomputed with the device SpMV.  Then, in a run of its own, one more
solve of each under the per-kernel event profile.

    python tools/bench_neumann.py --config C3 --base bj8
    python tools/bench_neumann.py --config C3 --base line_cyclic
    python tools/bench_neumann.py --config C4 --base line_product
    python tools/bench_neumann.py --config C1 --base line_jacobi

Prints one JSON line and appends it to profiles/neumann_bench.jsonl.  Reads nothing outside the
repository.  Needs the GPU: no fallback.  One process per configuration."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vt-precondition_amd")]

SEG = 25


def make_base(vk, A, prm, base):
    if base == "bj8":
        return vk.block_jacobi(A, 8)
    stride = vk.vlasov_line_stride(prm)
    if base == "line_jacobi":
        return vk.line_jacobi(A, stride, SEG)
    if base == "line_cyclic":
        return vk.line_cyclic(A, stride, vk.vlasov_line_period(prm), SEG)
    dirs = vk.vlasov_line_directions(prm)
    return vk.line_product(A, (dirs[0], SEG), (dirs[1], SEG))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3", choices=["C1", "C2", "C3", "C4", "S2", "S4"])
    ap.add_argument("--base", default="bj8", choices=["bj8", "line_jacobi", "line_cyclic", "line_product"])
    ap.add_argument("--degrees", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=15, help="restart cycles per solve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neumann_bench.jsonl"))
    a = ap.parse_args()
    degrees = [int(v) for v in a.degrees.split(",")]
    import torch   # first: one HIP runtime for torch and the library

    import vtkrylov as vk
    from oracle import twin
    vk._abi.check_build_id()
    if vk.device_count() < 1:
        raise SystemExit("bench_neumann: no HIP device (measurements need the GPU)")
    ctx = vk.default_context(0)
    p = twin.CONFIGS[a.config]
    prm = vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, vmax=p.vmax, E0=p.E0, nu=p.nu, alpha=p.alpha, cfl=p.cfl)
    A = vk.vlasov_operator(prm, ctx=ctx)
    M = make_base(vk, A, prm, a.base)
    prec = {k: (M if k == 1 else vk.neumann(A, M, k)) for k in degrees}
    n = A.n_local
    b = torch.from_numpy(vk.rhs_splitmix(n)).to(torch.device("cuda", 0))
    bnorm = float(torch.linalg.vector_norm(b))

    def solve(k):
        x, info = vk.gmres(A, b, rtol=a.rtol, restart=20, maxiter=a.maxiter, M=prec[k])
        st = vk.last_stats()
        res = float(torch.linalg.vector_norm(b - A.matvec(x))) / bnorm
        return {"info": info, "iterations": st.inner_iters, "restarts": st.restarts, "t": st.t_solve,
                "true_resid_over_bnorm": res, "orth": st.orth, "band": st.band, "bytes_moved": st.bytes_moved}

    warm = {k: solve(k) for k in degrees}   # warm-up: code objects, workspace; and which degrees converge
    timed = [k for k in degrees if warm[k]["info"] == 0]
    res = {k: [] for k in timed}
    for _ in range(a.reps):
        for k in timed:
            res[k].append(solve(k))
    out = {"tool": "bench_neumann", "config": a.config, "base": a.base, "n": n, "nnz": A.nnz, "fp32": bool(p.fp32),
           "rtol": a.rtol, "restart": 20, "maxiter": a.maxiter, "reps": a.reps, "layout": A.layout, "seg": SEG,
           "info": {str(k): (prec[k].info() if k > 1 else None) for k in degrees}, "degrees": {}}
    for k in degrees:
        if k not in res:
            w = warm[k]
            out["degrees"][str(k)] = {"converged": False, **{q: w[q] for q in w if q != "t"}, "ms_one_solve": round(w["t"] * 1e3, 4)}
            continue
        rr, last = res[k], res[k][-1]
        out["degrees"][str(k)] = {"converged": True, "ms_median": round(statistics.median(r["t"] for r in rr) * 1e3, 4),
                                  "ms": [round(r["t"] * 1e3, 4) for r in rr], **{q: last[q] for q in last if q != "t"}}
    if 1 in res:
        t1, i1 = out["degrees"]["1"]["ms_median"], out["degrees"]["1"]["iterations"]
        out["over_base"] = {str(k): {"ms": round(out["degrees"][str(k)]["ms_median"] / t1, 4),
                                     "iterations": round(out["degrees"][str(k)]["iterations"] / i1, 4)}
                            for k in timed if k != 1}
    prof = {}
    for k in timed:   # a run of its own: the events serialise the launches
        ctx.profile(True)
        solve(k)
        pr = ctx.profile_read()
        ctx.profile(False)
        prof[str(k)] = {c: {"launches": v["launches"], "avg_us": round(v["avg_us"], 2), "gbs": round(v["gbs"], 1)}
                        for c, v in sorted(pr.items(), key=lambda kv: -kv[1]["seconds"])}
    out["kernels"] = prof
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(out) + "\n")
    for k in degrees:
        if k > 1:
            prec[k].close()
    M.close()
    A.close()


if __name__ == "__main__":
    main()
