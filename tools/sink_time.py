"""Time DeviceAssembler.sinking + add_matrix over a year of slots (csrc/otmb_sink.hip, csrc/otmb_addmat.hip) on the 1 degree preset against
the host route the parent commit offers; one JSON line per measurement.

    python tools/sink_time.py [--reps 7] [--host-reps 3] [--host-lib PATH] [--no-host] [--out FILE.jsonl]

The operator: T of the 1 degree preset and eleven copies scaled by 1 + 0.02·m in twelve value slots.  w: 100 m per day.
  device   S = sinking(w), then add_matrix(S) over all twelve slots: wall times with a wait for the device, medians of --reps after one
           warm-up; add_matrix(S, slots=0) beside it, so that (twelve slots - one slot) / 11 is a slot's share of the update kernel and the
           rest the checks, the match and the waits.  The update's bytes per slot: 2 arrays x 16 B x nnz(S) read and written, and once per
           call B's values, pos and dst (24 B x nnz(S)), against otmb_ctx_stream_mix over arrays of the same sizes.
  host     the route without add_matrix: to_csc of every slot (twelve downloads), scipy T_m + S, set_values(..., slot=m) twelve times.
           --host-lib: run it on another build of the library (the parent commit's), alternating with the device route."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import otmb_amd  # noqa: E402
import otmb_amd.api as api  # noqa: E402
from otmb_amd import capi, synthetic  # noqa: E402
from otmb_amd.device import DeviceAssembler  # noqa: E402

NSLOTS = 12
W = 100.0 / 86400.0


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def stats(t):
    return {"median_s": float(np.median(t)), "min_s": float(np.min(t)), "max_s": float(np.max(t))}


def host_route(p, i, months, S, lib_path):
    """One pass of the host route on an api.DeviceOperator of the library at lib_path (None: the one loaded): (download, scipy, upload) s."""
    import scipy.sparse as sp

    here = capi.LIB_PATH
    if lib_path:
        capi.use_library(lib_path, lenient=True)
        api._ctx.clear()
    N = len(p) - 1
    try:
        D = api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, months[0]))
        D.set_slots(NSLOTS)
        for m in range(1, NSLOTS):
            D.set_values(months[m], slot=m)
        Ss = sp.csc_matrix((S[2], S[1] - 1, S[0] - 1), shape=(N, N))
        t0 = time.perf_counter()
        got = [D.to_csc(m) for m in range(NSLOTS)]
        t1 = time.perf_counter()
        sums = []
        for A in got:
            C = sp.csc_matrix((A.nzval, A.rowval - 1, A.colptr - 1), shape=(N, N)) + Ss
            C.sort_indices()
            assert C.nnz == len(i)  # (no exact cancellation: the pattern is T's)
            sums.append(C.data)
        t2 = time.perf_counter()
        for m in range(NSLOTS):
            D.set_values(sums[m], slot=m)
        t3 = time.perf_counter()
        D.close()
    finally:
        if lib_path:
            api._ctx.clear()
            capi.use_library(here)
    return t1 - t0, t2 - t1, t3 - t2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-lib", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    g = synthetic.preset("access1deg", rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    N = asm.N
    op = asm.keep_slot(0, nslots=NSLOTS)
    nnz = op.nnz
    nz0 = asm.out["T"][2][:nnz]
    months = [(nz0 * (1.0 + 0.02 * m)).contiguous() for m in range(NSLOTS)]
    for m in range(NSLOTS):
        op.set_values_dev(months[m], slot=m)
    S = asm.sinking(W)
    nnzs = int(S[1].numel())
    base = {"n": N, "nnz": nnz, "nnz_S": nnzs, "nslots": NSLOTS}

    t_sink, t_all, t_one, t_host = [], [], [], []
    hp = hi = hm = hs = None
    if not a.no_host:
        hp, hi = asm.out["T"][0].cpu().numpy(), asm.out["T"][1][:nnz].cpu().numpy()
        hm = [m.cpu().numpy() for m in months]
        hs = tuple(x.cpu().numpy() for x in S)
    for rep in range(a.reps + 1):  # alternating: the device route, then (for the first --host-reps + 1 rounds) the host route
        ts, S = wall(lambda: asm.sinking(W))
        ta, _ = wall(lambda: op.add_matrix(S))
        to, _ = wall(lambda: op.add_matrix(S, slots=0))
        if rep:
            t_sink.append(ts), t_all.append(ta), t_one.append(to)
        if not a.no_host and rep <= a.host_reps:
            h = host_route(hp, hi, hm, hs, a.host_lib)
            if rep:
                t_host.append(h)
    per_slot = max(float(np.median(t_all)) - float(np.median(t_one)), 0.0) / (NSLOTS - 1)
    slot_bytes = 2 * 16 * nnzs
    emit(dict(base, what="device: sinking + add_matrix over twelve slots", sinking=stats(t_sink), add_matrix_twelve=stats(t_all), add_matrix_one=stats(t_one),
              total_median_s=float(np.median(t_sink) + np.median(t_all)), update_per_slot_s=per_slot, update_bytes_per_slot=slot_bytes,
              update_bytes_once_per_call=24 * nnzs, update_gbs=(slot_bytes / per_slot / 1e9) if per_slot > 0 else None, reps=a.reps))
    # the stream's rate over arrays of the update's sizes: per slot nz and val read and written (16 B x nnz(S) each way), B's values, pos and dst read
    f = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
    ins = [f(2 * nnzs) for _ in range(NSLOTS)] + [f(nnzs) for _ in range(3)]
    outs = [f(2 * nnzs) for _ in range(NSLOTS)]
    for t in ins:
        t.zero_()
    torch.cuda.synchronize()
    gbs = [asm.ctx.stream_mix([(t.data_ptr(), t.numel() * 8) for t in ins], [(t.data_ptr(), t.numel() * 8) for t in outs], max((nnzs + 2047) // 2048, 1))
           for _ in range(4)][1:]
    emit(dict(base, what="otmb_ctx_stream_mix over arrays of the update's sizes", bytes=int(sum(t.numel() for t in ins + outs) * 8), median_gbs=float(np.median(gbs)), min_gbs=float(np.min(gbs)), max_gbs=float(np.max(gbs))))
    if t_host:
        emit(dict(base, what="host route: twelve to_csc, scipy T_m + S, twelve set_values", library=a.host_lib or "this build",
                  downloads=stats([h[0] for h in t_host]), scipy_sums=stats([h[1] for h in t_host]), uploads=stats([h[2] for h in t_host]),
                  total=stats([sum(h) for h in t_host]), reps=len(t_host)))


if __name__ == "__main__":
    main()
