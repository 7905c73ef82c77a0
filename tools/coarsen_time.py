#!/usr/bin/env python3
"""Time coarsen (C = LUMP * T * SPRAY, csrc/otmb_coarsen.hip) at 1 degree with 2 x 2 x 1 blocks, without a mask and with the
reference's SO / NA mask (test/online.jl:126-128).  GPU only.  Prints one JSON line:
  device   plan + fill of DeviceAssembler.coarsen on the resident T, from HIP events, after warm-up (median of --reps)
  host     api.coarsen wall time, and what its upload / download of the same bytes cost alone (pageable torch copies)
  scipy    (L @ T) @ S on this host
  bytes    algorithmic: the three CSC matrices read once per pass (plan, fill), the result written once.
python tools/coarsen_time.py [--workload access1deg] [--reps 50]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="access1deg")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("coarsen_time.py needs a GPU")
    import otmb_amd
    import otmb_amd.api as api
    from otmb_amd import synthetic
    from otmb_amd.device import DeviceAssembler

    g = synthetic.preset(args.workload, rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    host = asm.result_to_host()
    N, nz = asm.N, asm.nz
    lat, lon = np.asarray(g.lat), np.asarray(g.lon) % 360
    so, na = lat < -35, (lat > 50) & ((lon < 100) | (250 < lon))
    somask = np.repeat((~so & ~na)[:, :, None], nz, axis=2)
    T = api.SparseMatrixCSC(N, N, *host["T"])
    Tm = T.to_scipy()
    out = {"workload": args.workload, "N": N, "nnz_T": T.nnz, "device": torch.cuda.get_device_name(0), "cases": []}
    for label, mask in (("2x2x1", None), ("2x2x1 SO/NA mask", somask)):
        dm = None if mask is None else torch.from_numpy(np.asfortranarray(mask).ravel(order="F").astype(np.uint8)).cuda()
        L, S, vc = asm.lump_and_spray(dm, 2, 2, 1)
        Nc = len(vc)
        for _ in range(5):
            Cp, Ci, Cx = asm.coarsen(L, S)
        torch.cuda.synchronize()
        dev = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            Cp, Ci, Cx = asm.coarsen(L, S)
            e1.record()
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        nnz = Ci.numel()
        Lh = api.SparseMatrixCSC(Nc, N, *(t.cpu().numpy() for t in L))
        Sh = api.SparseMatrixCSC(N, Nc, *(t.cpu().numpy() for t in S))
        api.coarsen(Lh, T, Sh)
        hw = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            C = api.coarsen(Lh, T, Sh)
            hw.append(time.perf_counter() - t0)
        ins = [x for X in (Lh, T, Sh) for x in (X.colptr, X.rowval, X.nzval)]
        up, down = [], []
        for _ in range(args.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in ins]
            torch.cuda.synchronize()
            up.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for t in (Cp, Ci, Cx):
                t.cpu()
            down.append(time.perf_counter() - t0)
            del ds
        t0 = time.perf_counter()
        ref = (Lh.to_scipy() @ Tm) @ Sh.to_scipy()
        tsci = time.perf_counter() - t0
        same = np.array_equal(C.colptr, Cp.cpu().numpy()) and np.array_equal(C.rowval, Ci.cpu().numpy()) and \
            np.array_equal(np.asarray(C.nzval).view(np.int64), Cx.cpu().numpy().view(np.int64))
        in_bytes = sum(int(np.asarray(x).nbytes) for x in ins)
        out_bytes = (Nc + 1) * 8 + nnz * 16
        bytes_ = 2 * in_bytes + out_bytes
        dmed = statistics.median(dev)
        out["cases"].append({
            "case": label, "Nc": Nc, "nnz_C": nnz, "scipy_nnz": int(ref.nnz),
            "device_ms_median": round(dmed, 4), "device_ms_min": round(min(dev), 4), "device_ms_max": round(max(dev), 4),
            "host_ms_median": round(1e3 * statistics.median(hw), 3), "host_upload_ms": round(1e3 * statistics.median(up), 3),
            "host_download_ms": round(1e3 * statistics.median(down), 3), "scipy_ms": round(1e3 * tsci, 2),
            "algorithmic_bytes": bytes_, "algorithmic_GBps": round(bytes_ / (dmed * 1e-3) / 1e9, 1),
            "host_equals_device": bool(same), "reps": args.reps})
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
