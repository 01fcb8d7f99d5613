"""What a time step pays to change the operator's values: rebuild against update.

In one process, after a warm-up of both, two paths alternate `--reps` times each, a device
synchronise around every timed region, the Vlasov parameters toggling between two sets so that the
values really change every step:

  (a) rebuild:  destroy M and A, vlasov_operator(p), block_jacobi(A, 8)
  (b) update:   A.update_vlasov(p), M.refresh()

then one more (b) under the per-kernel event profile (classes sell_refresh, vlasov_values,
lsv_build / grid4_build, bj_setup, bj_tri_setup: algorithmic bytes / event time).  With --host-arrays (C3 by
default) the same through the drop-in path: csr_matrix((data, indices, indptr)) + block_jacobi
against update_values(data) + refresh, from host arrays.

    python tools/bench_update.py [--configs C3 C4] [--reps 5] [--host-arrays C3] [--out-dir profiles]

Prints one JSON line per config and writes <out-dir>/update_values_<config in lower case>.json.  The requirement
it checks ("pass"): (b)'s median below the fastest of (a)'s runs.  Needs the GPU: no fallback."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vt-precondition_amd")]

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12   # B/s: datasheet peak, measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C3", "C4"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-arrays", nargs="*", default=["C3"], help="configs also run through csr_matrix / update_values")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch   # first: one HIP runtime for torch and the library

    import vtkrylov as vk
    from oracle import twin
    vk._abi.check_build_id()
    if vk.device_count() < 1:
        raise SystemExit("bench_update: no HIP device (measurements need the GPU)")
    ctx = vk.default_context(0)
    dev = torch.device("cuda", 0)

    def timed(fn):
        ctx.synchronize()
        t = time.perf_counter()
        out = fn()
        ctx.synchronize()
        return time.perf_counter() - t, out

    for name in a.configs:
        p = twin.CONFIGS[name]
        ps = [p, dataclasses.replace(p, cfl=8.0, E0=0.8, nu=0.1)]
        prm = [vk.vlasov_params(q.dim, q.shape, fp32=q.fp32, vmax=q.vmax, E0=q.E0, nu=q.nu, alpha=q.alpha, cfl=q.cfl)
               for q in ps]
        x = torch.from_numpy(twin.rhs(p.n, seed=0xC0FFEE)).to(dev)
        state = {}

        def rebuild(k):
            for o in ("M", "A"):
                if o in state:
                    state.pop(o).close()
            state["A"] = vk.vlasov_operator(prm[k], ctx=ctx)
            state["M"] = vk.block_jacobi(state["A"], 8)

        def update(k):
            t0 = time.perf_counter()
            state["A"].update_vlasov(prm[k])
            ctx.synchronize()
            t1 = time.perf_counter()
            state["M"].refresh()
            ctx.synchronize()
            return t1 - t0, time.perf_counter() - t1

        rebuild(0)       # warm-up of both paths (code objects, allocator)
        update(1)
        rebuild(0)
        update(1)
        ta, tb, tbu, tbr = [], [], [], []
        k = 0
        for _ in range(a.reps):
            t, _ = timed(lambda: rebuild(k))
            ta.append(t)
            k ^= 1
            t, (tu, tr) = timed(lambda: update(k))
            tb.append(t)
            tbu.append(tu)
            tbr.append(tr)
            k ^= 1
        # the updated operator against a fresh one: the same SpMV bits (the tests' rule, at this size)
        y = state["A"] @ x
        F = vk.vlasov_operator(prm[k ^ 1], ctx=ctx)
        same = bool(torch.equal(y, F @ x))
        tabs = (state["A"].line_band, state["A"].line_values) + state["A"].grid4
        same = same and tabs == (F.line_band, F.line_values) + F.grid4
        F.close()
        # one profiled update + refresh: per-kernel rates
        ctx.profile(True)
        update(k)
        prof = ctx.profile_read()
        ctx.profile(False)
        li = state["A"].layout_info()
        n, nnz = state["A"].n_local, state["A"].nnz
        bytes_b = sum(v["bytes"] for v in prof.values())
        kern_s = sum(v["seconds"] for v in prof.values())
        b_med = statistics.median(tb)
        res = {"tool": "bench_update", "config": name, "n": n, "nnz": nnz, "fp32": bool(p.fp32), "reps": a.reps,
               "layout": li["layout"], "sell_entries": li["sell_entries"], "tables": list(tabs),
               "rebuild_s": [round(t, 6) for t in ta], "update_s": [round(t, 6) for t in tb],
               "update_values_s": [round(t, 6) for t in tbu], "refresh_s": [round(t, 6) for t in tbr],
               "rebuild_min_s": min(ta), "rebuild_median_s": statistics.median(ta), "update_median_s": b_med,
               "speedup_median": statistics.median(ta) / b_med, "pass": bool(b_med < min(ta)),
               "spmv_and_tables_equal_fresh": same,
               "kernels": {c: {"launches": v["launches"], "avg_us": round(v["avg_us"], 1), "gbs": round(v["gbs"], 1),
                               "bytes": v["bytes"]} for c, v in sorted(prof.items(), key=lambda kv: -kv[1]["seconds"])},
               "byte_model": {"bytes": bytes_b, "kernel_seconds": kern_s,
                              "s_at_8.0TBs": bytes_b / HBM_SPEC, "s_at_6.29TBs": bytes_b / HBM_COPY,
                              "kernel_seconds_over_model_6.29": kern_s / (bytes_b / HBM_COPY) if bytes_b else None,
                              "update_median_over_model_6.29": b_med / (bytes_b / HBM_COPY) if bytes_b else None,
                              "note": "algorithmic bytes of the profiled classes of one update + refresh; "
                                      "6.29 TB/s = measured float4 copy, 8.0 TB/s = datasheet"}}
        if name in (a.host_arrays or []):
            cur = k   # the parameter set of A's values (the profiled update above)
            ip, ix, d_cur = state["A"].download()
            state["A"].update_vlasov(prm[cur ^ 1])
            hd = {cur: d_cur, cur ^ 1: state["A"].download()[2]}   # host values per parameter set
            hs = {}

            def h_rebuild(j):
                for o in ("M", "A"):
                    if o in hs:
                        hs.pop(o).close()
                hs["A"] = vk.csr_matrix((hd[j], ix, ip), shape=(p.n, p.n), ctx=ctx)
                hs["M"] = vk.block_jacobi(hs["A"], 8)

            def h_update(j):
                hs["A"].update_values(hd[j])
                hs["M"].refresh()

            h_rebuild(0)   # warm-up
            h_update(1)
            ha, hb = [], []
            j = 0
            for _ in range(a.reps):
                ha.append(timed(lambda: h_rebuild(j))[0])
                j ^= 1
                hb.append(timed(lambda: h_update(j))[0])
                last = j
                j ^= 1
            Fh = vk.vlasov_operator(prm[last], ctx=ctx)
            same_h = bool(torch.equal(hs["A"] @ x, Fh @ x)) and hs["A"].line_values == Fh.line_values
            Fh.close()
            res["host_arrays"] = {"rebuild_s": [round(t, 6) for t in ha], "update_s": [round(t, 6) for t in hb],
                                  "rebuild_min_s": min(ha), "update_median_s": statistics.median(hb),
                                  "speedup_median": statistics.median(ha) / statistics.median(hb),
                                  "pass": bool(statistics.median(hb) < min(ha)),
                                  "spmv_and_tables_equal_fresh": same_h,
                                  "h2d_bytes_per_update": int(d_cur.nbytes)}
            for o in ("M", "A"):
                hs.pop(o).close()
        for o in ("M", "A"):
            state.pop(o).close()
        print(json.dumps(res))
        os.makedirs(a.out_dir, exist_ok=True)
        with open(os.path.join(a.out_dir, f"update_values_{name.lower()}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
