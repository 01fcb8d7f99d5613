"""Path ledger: which launches each solver configuration issues (tests/test_gpu_path_ledger.py).

For every row of the tables below one solve of fixed length runs under the per-kernel event
profile -- a tolerance no cycle can meet, ``maxiter=2`` restart cycles (BiCGStab: BCG_ITERS
iterations) -- and one record is kept: per profile class its launch count and its byte total (the
host's algorithmic figure, a double), and ``band``, ``orth``, ``inner_iters``, ``restarts``,
``info`` of the solve (``solver="apply"``: one ``M @ b``; ``"precond_matvec"``: one ``M^-1 A b``; their records
are the classes alone).  The records of the committed library are tests/golden/path_ledger.json;
the test replays the tables and compares with ``==``.  A change of the host driver that moves a
configuration to another path, or changes a launch count or a byte model, shows up as a diff of
that file and is re-recorded on purpose:

    python tools/record_path_ledger.py [--out tests/golden/path_ledger.json] [--bits FILE]

--bits FILE: also write, per row, the SHA-256 of x and rnorm / presid as hex floats to FILE (a
one-off comparison of two host drivers over the same device code; not part of the fixture: a
kernel change moves these legitimately).

Needs the GPU: no fallback.  Reads nothing outside the repository."""
import argparse
import hashlib
import json
import os
import socket
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "vt-precondition_amd")) if p not in sys.path]

import numpy as np  # noqa: E402

from oracle import twin  # noqa: E402

NOSTOP = 1e-30     # rtol no cycle can meet: every column of every cycle runs
BCG_ITERS = 6
X0_SEED = 0xB00
NU_LAGGED = 0.06   # the value update of the lagged-M row (vlasov_params' default nu is 0.05)


def _row(id, op, prec=None, solver="gmres", restart=20, tune=None, layout=None, mode="auto", x0=False, orth=None,
         lagged=False, band=None):
    return dict(id=id, op=op, prec=prec, solver=solver, restart=restart, tune=tune or {}, layout=layout, mode=mode,
                x0=x0, orth=orth, lagged=lagged, band=band)


BJ8, LINE, LINE2 = ("bj", 8), ("line", 8), ("line2", 8, 8)
LINE64, LINEC, SPAN = ("line", 64), ("linec", 8), ("linec_span", 8)   # seg 64 > 32: no register sweeps (no line_dc kernel)
# line rows: restart 6 (a line-preconditioned cycle of 20 columns reaches rounding on S2); 4D: 10
ROWS = [
    # S2 + BJ(8): the band step with the ring start, and each switch that leaves part of it
    _row("s2_bj8_m20", "S2", BJ8, band=1),
    _row("s2_bj8_m3", "S2", BJ8, restart=3, band=1),
    _row("s2_bj8_long_rows0", "S2", BJ8, tune={"band_long_rows": 0}, band=1),
    _row("s2_bj8_band0", "S2", BJ8, tune={"band": 0}, band=0),
    _row("s2_bj8_band_lsv0", "S2", BJ8, tune={"band_lsv": 0}, band=1),
    _row("s2_bj8_cyc_ring0", "S2", BJ8, tune={"cyc_ring": 0}, band=1),
    _row("s2_bj4", "S2", ("bj", 4), band=0),
    _row("s2_bj16", "S2", ("bj", 16), band=0),
    _row("s2_bj8_inverse", "S2", BJ8, mode="inverse", band=0),
    _row("s2_none", "S2", None, band=0),
    _row("s2_bj8_csr", "S2", BJ8, layout="csr", band=0),
    _row("s2_bj8_lagged", "S2", BJ8, lagged=True, band=0),   # values updated, no refresh: leaves the band
    _row("s2_line_fuse1", "S2", LINE, restart=6, tune={"line_fuse": 1}, band=0),
    _row("s2_line_fuse0", "S2", LINE, restart=6, tune={"line_fuse": 0}, band=0),
    _row("s2_line_band_lsv0", "S2", LINE, restart=6, tune={"band_lsv": 0}, band=0),
    _row("s2_line2_dc1", "S2", LINE2, restart=6, tune={"line2_dc": 1}, band=0),
    _row("s2_line2_dc0", "S2", LINE2, restart=6, tune={"line2_dc": 0}, band=0),
    _row("s4_bj8_ring64", "S4", BJ8, restart=10, tune={"g4_ring": 64}, band=0),
    _row("s4_bj8_ring0_fused1", "S4", BJ8, restart=10, tune={"g4_ring": 0, "c4_fused": 1}, band=0),
    _row("s4_bj8_ring0_fused0", "S4", BJ8, restart=10, tune={"g4_ring": 0, "c4_fused": 0}, band=0),
    _row("s4f_bj8", "S4F", BJ8, restart=10, band=0),
    # each family with x0 != 0: the cycle-start residual of cycle 0 too
    _row("s2_bj8_x0", "S2", BJ8, x0=True, band=1),
    _row("s2_bj4_x0", "S2", ("bj", 4), x0=True),
    _row("s2_none_x0", "S2", None, x0=True),
    _row("s2_line_x0", "S2", LINE, restart=6, x0=True),
    _row("s2_line_cyc_ring0_x0", "S2", LINE, restart=6, tune={"cyc_ring": 0}, x0=True),
    _row("s2_line2_x0", "S2", LINE2, restart=6, x0=True),
    _row("s4_bj8_ring64_x0", "S4", BJ8, restart=10, tune={"g4_ring": 64}, x0=True),
    _row("s4f_bj8_x0", "S4F", BJ8, restart=10, x0=True),
    _row("s2_bj8_mgs", "S2", BJ8, orth="mgs", band=0),
    _row("bcg_s2_none", "S2", None, solver="bicgstab"),
    _row("bcg_s2_bj8_fuse1", "S2", BJ8, solver="bicgstab", tune={"bcg_fuse": 1}),
    _row("bcg_s2_bj8_fuse0", "S2", BJ8, solver="bicgstab", tune={"bcg_fuse": 0}),
    _row("bcg_s2_line", "S2", LINE, solver="bicgstab"),
    _row("pmv_s2_bj8", "S2", BJ8, solver="precond_matvec"),
    _row("pmv_s2_line", "S2", LINE, solver="precond_matvec"),
    _row("pmv_s4_bj8_ring64", "S4", BJ8, solver="precond_matvec", tune={"g4_ring": 64}),
    # the cyclic lines (three phases, then the dots kernel) and line Jacobi through the generic step
    _row("s2_linec", "S2", LINEC, restart=6, band=0),
    _row("s2_linec_band_lsv0", "S2", LINEC, restart=6, tune={"band_lsv": 0}, band=0),
    _row("s2_linec_x0", "S2", LINEC, restart=6, x0=True),
    _row("s2_line64", "S2", LINE64, restart=6, band=0),
    # the Neumann wrapper: the fused correction (BJ-fused tiles, bs <= 8), else residual + the base's
    # launches with the addend; the step's dots behind the last write (neu_dc) where the kind has that form
    _row("s2_neu2_bj8", "S2", ("neu", 2, BJ8), restart=6, band=0),
    _row("s2_neu2_bj8_fuse0", "S2", ("neu", 2, BJ8), restart=6, tune={"neu_fuse": 0}, band=0),
    _row("s2_neu2_bj8_fuse0_dc0", "S2", ("neu", 2, BJ8), restart=6, tune={"neu_fuse": 0, "neu_dc": 0}, band=0),
    _row("s2_neu2_bj16", "S2", ("neu", 2, ("bj", 16)), restart=6, band=0),
    _row("s2_neu2_line", "S2", ("neu", 2, LINE), restart=6, band=0),
    _row("s2_neu2_line_dc0", "S2", ("neu", 2, LINE), restart=6, tune={"neu_dc": 0}, band=0),
    _row("s2_neu2_line64", "S2", ("neu", 2, LINE64), restart=6, band=0),
    _row("s2_neu2_line2", "S2", ("neu", 2, LINE2), restart=6, band=0),
    _row("s2_neu2_line2_dc0", "S2", ("neu", 2, LINE2), restart=6, tune={"neu_dc": 0}, band=0),
    _row("s2_neu2_linec", "S2", ("neu", 2, LINEC), restart=6, band=0),
    _row("s2_neu3_line2", "S2", ("neu", 3, LINE2), restart=6, band=0),
    _row("s2_neu1_bj8", "S2", ("neu", 1, BJ8), restart=6, band=0),
    _row("s2_neu2_line2_x0", "S2", ("neu", 2, LINE2), restart=6, x0=True),
    _row("bcg_s2_line2", "S2", LINE2, solver="bicgstab"),
    _row("bcg_s2_linec", "S2", LINEC, solver="bicgstab"),
    _row("bcg_s2_neu2_bj8", "S2", ("neu", 2, BJ8), solver="bicgstab"),
    _row("bcg_s2_neu2_line", "S2", ("neu", 2, LINE), solver="bicgstab"),
    _row("pmv_s2_line2", "S2", LINE2, solver="precond_matvec"),
    _row("pmv_s2_linec", "S2", LINEC, solver="precond_matvec"),
    _row("pmv_s2_neu2_bj8", "S2", ("neu", 2, BJ8), solver="precond_matvec"),
    # one standalone M @ b per kind
    _row("app_s2_bj8", "S2", BJ8, solver="apply"),
    _row("app_s2_bj8_inverse", "S2", BJ8, solver="apply", mode="inverse"),
    _row("app_s2_line", "S2", LINE, solver="apply"),
    _row("app_s2_line2", "S2", LINE2, solver="apply"),
    _row("app_s2_linec", "S2", LINEC, solver="apply"),
    _row("app_s2_neu3_line2", "S2", ("neu", 3, LINE2), solver="apply"),
]

# across ranks (host-staged communicator, the ranks share the GPU): one spawn per group
RANK_GROUPS = {
    "S2_w2": (2, [_row("s2_bj8_m20", "S2", BJ8, band=1), _row("s2_bj8_m3", "S2", BJ8, restart=3, band=1),
                  _row("bcg_s2_bj8", "S2", BJ8, solver="bicgstab"),
                  _row("s2_linec_span", "S2", SPAN, restart=6, band=0),
                  _row("bcg_s2_linec_span", "S2", SPAN, solver="bicgstab"),
                  _row("app_s2_linec_span", "S2", SPAN, solver="apply"),
                  _row("s2_neu2_bj8", "S2", ("neu", 2, BJ8), restart=6, band=0)]),
    "S2_w3": (3, [_row("s2_bj8_m20", "S2", BJ8, band=1), _row("s2_bj8_m3", "S2", BJ8, restart=3, band=1),
                  _row("s2_linec_span", "S2", SPAN, restart=6, band=0)]),
    "S4_w2": (2, [_row("s4_bj8_ring64", "S4", BJ8, restart=10, tune={"g4_ring": 64}, band=0),
                  _row("s4_bj8", "S4", BJ8, restart=10, band=0),
                  _row("pmv_s4_bj8_ring64", "S4", BJ8, solver="precond_matvec", tune={"g4_ring": 64})]),
    "S4_w3": (3, [_row("s4_bj8_ring64", "S4", BJ8, restart=10, tune={"g4_ring": 64}, band=0),
                  _row("s4_bj8", "S4", BJ8, restart=10, band=0),
                  _row("pmv_s4_bj8_ring64", "S4", BJ8, solver="precond_matvec", tune={"g4_ring": 64})]),
}


def _prec(vk, A, p, prec, mode):
    if prec is None:
        return None
    if prec[0] == "bj":
        return vk.block_jacobi(A, prec[1], mode=mode)
    if prec[0] == "neu":   # ("neu", degree, base): the wrapper keeps its base (run_row closes both)
        return vk.neumann(A, _prec(vk, A, p, prec[2], mode), prec[1])
    vp = vk.vlasov_params(p.dim, p.shape)
    if prec[0] in ("linec", "linec_span"):
        return vk.line_cyclic(A, vk.vlasov_line_stride(vp), vk.vlasov_line_period(vp), prec[1], span=prec[0] == "linec_span")
    sx, sv = vk.vlasov_line_directions(vp)[:2]
    if prec[0] == "line":
        return vk.line_jacobi(A, sx, prec[1])
    return vk.line_product(A, (sx, prec[1]), (sv, prec[2]))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_row(vk, ctx, row, offsets=None):
    """(record, bits) of one row on ``ctx`` (``offsets``: this rank's slab of a distributed operator)."""
    p = twin.CONFIGS[row["op"]]
    A = vk.vlasov_operator(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32), ctx=ctx, offsets=offsets)
    if row["layout"]:
        A.set_layout(row["layout"])
    M = _prec(vk, A, p, row["prec"], row["mode"])
    try:
        if row["lagged"]:
            A.update_vlasov(vk.vlasov_params(p.dim, p.shape, fp32=p.fp32, nu=NU_LAGGED))
        rb, re_ = A.row_begin, A.row_end
        b = twin.rhs(p.n)[rb:re_]
        x0 = twin.rhs(p.n, seed=X0_SEED)[rb:re_] * 1e-3 if row["x0"] else None
        with ctx.tuning(**row["tune"]):
            ctx.profile(True)
            try:
                if row["solver"] == "gmres":
                    x, info = vk.gmres(A, b, x0=x0, rtol=NOSTOP, M=M, restart=row["restart"], maxiter=2, orth=row["orth"])
                    st = vk.last_stats()
                    rec = dict(band=st.band, orth=st.orth, inner_iters=st.inner_iters, restarts=st.restarts, info=info)
                    bits = dict(x=_sha(x), rnorm=float(st.rnorm).hex(), presid=float(st.presid).hex())
                elif row["solver"] == "bicgstab":
                    x, info = vk.bicgstab(A, b, x0=x0, rtol=NOSTOP, M=M, maxiter=BCG_ITERS)
                    st = vk.last_bicgstab_stats()
                    rec = dict(iterations=st.iterations, half_step=st.half_step, info=info)
                    bits = dict(x=_sha(x), rnorm=float(st.rnorm).hex())
                elif row["solver"] == "apply":
                    z = M @ b
                    rec, bits = {}, dict(x=_sha(z))
                else:
                    w = A.precond_matvec(M, b)
                    rec, bits = {}, dict(x=_sha(w))
                rec["classes"] = {k: [e["launches"], e["bytes"]] for k, e in sorted(ctx.profile_read().items())}
            finally:
                ctx.profile(False)
    finally:
        if M is not None:
            M.close()
            if getattr(M, "base", None) is not None:
                M.base.close()
        A.close()
    return rec, bits


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, group, outdir):
    import datetime
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    import vtkrylov as vk
    ctx = vk.Context(0)
    hc = ctx.comm_init_host(rank, world)
    out = {}
    for row in RANK_GROUPS[group][1]:
        p = twin.CONFIGS[row["op"]]
        offs = vk.partition_rows(p.n, world, p.shape[-1] if p.dim == 2 else int(np.prod(p.shape[1:])))
        out[row["id"]] = run_row(vk, ctx, row, offs)
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(dict(rows=out, errors=[str(e) for e in hc.errors]), f)
    dist.barrier()
    dist.destroy_process_group()


def run_group(group):
    """{row id: [(record, bits) of rank 0, of rank 1, ...]} of one spawn."""
    import torch.multiprocessing as mp
    world = RANK_GROUPS[group][0]
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_rank_worker, args=(world, _free_port(), group, d), nprocs=world, join=True)
        z = []
        for r in range(world):
            with open(os.path.join(d, f"rank{r}.json")) as f:
                z.append(json.load(f))
    for q in z:
        assert not q["errors"], q["errors"]
    return {row["id"]: [q["rows"][row["id"]] for q in z] for row in RANK_GROUPS[group][1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "path_ledger.json"))
    ap.add_argument("--bits", default=None, help="also write x hashes and norms here (one-off comparison)")
    a = ap.parse_args()
    import vtkrylov as vk
    vk._abi.check_build_id()
    ctx = vk.default_context(0)
    led, bits = {"rows": {}, "ranks": {}}, {"rows": {}, "ranks": {}}
    for row in ROWS:
        led["rows"][row["id"]], bits["rows"][row["id"]] = run_row(vk, ctx, row)
        print(row["id"], json.dumps(led["rows"][row["id"]]), flush=True)
    for group in RANK_GROUPS:
        got = run_group(group)
        led["ranks"][group] = {k: [rb[0] for rb in v] for k, v in got.items()}
        bits["ranks"][group] = {k: [rb[1] for rb in v] for k, v in got.items()}
        print(group, json.dumps(led["ranks"][group]), flush=True)
    for path, obj in ((a.out, led), (a.bits, bits)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(obj, f, indent=1, sort_keys=True)
                f.write("\n")
            print("wrote", path)


if __name__ == "__main__":
    main()
