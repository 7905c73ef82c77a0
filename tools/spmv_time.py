"""Time the resident sparse operator (otmb_op_*, csrc/otmb_spmv.hip) on T of the 1 degree preset; one JSON line per measurement.

    python tools/spmv_time.py [--reps 50] [--out FILE.jsonl]

Device times are HIP events around each call on the context's stream (torch.cuda.Event on the same stream), the median of --reps after
warm-up.  Algorithmic bytes (what each call must move at the least, every array once):
    A·x    12 nnz (values + Int32 columns of the row layout) + 4 m (row lengths) + 8 n (x) + 8 m (y written; β = 0)
    Aᵀ·x   12 nnz (nzval + Int32 rows of the CSC copy) + 8 (n + 1) (colptr) + 8 m (x) + 8 n (y)
    A·X    k tracers: 12 nnz + 4 m + 8 k (n + m)   (the matrix read once per register block of up to 8 tracers)
    set    8 nnz copied in (read + write) + 8 nnz (the copy) + 8 nnz (positions) read + 8 nnz written: 40 nnz
    plan   not a streaming pass (a radix sort and scans): time only
The share of HBM peak is bytes / time / 8 TB/s.  "stream_ratio": the time of otmb_ctx_stream_mix -- the plainest kernel over arrays of
the same byte mix in this process (T's nzval and half of its rowval as the matrix streams, x, y) -- over the call's time (1.0: as fast as
an ideal stream).  "host_route": the parent's only way to apply T, result_to_host of T then scipy's T @ x on the host."""
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
from otmb_amd import synthetic  # noqa: E402
from otmb_amd.device import DeviceAssembler, Operator  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = synthetic.preset("access1deg", rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    N, nnz = asm.N, asm.nnz[0]
    cp, rv, nz = asm.out["T"]
    lines = []

    def emit(what, t, nbytes, stream_s=None, **extra):
        rec = {"what": what, "N": N, "nnz": nnz, "median_s": t[0], "min_s": t[1], "max_s": t[2], "reps": a.reps}
        if nbytes is not None:
            rec.update(bytes=int(nbytes), gbs=nbytes / t[0] / 1e9, share_of_peak=nbytes / t[0] / PEAK)
        if stream_s is not None:
            rec.update(stream_mix_s=stream_s, stream_ratio=stream_s / t[0])
        rec.update(extra)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    # plan (create) and set values
    op = Operator(asm.ctx, N, N, cp, rv, nz)
    t_plan = timed(lambda: Operator(asm.ctx, N, N, cp, rv, nz).close(), max(5, a.reps // 10), warm=1)
    emit("plan (otmb_op_create_dev + destroy)", t_plan, None)
    emit("set_values_dev", timed(lambda: op.set_values_dev(nz), a.reps), 40 * nnz)
    x = torch.randn(N, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    X8 = torch.randn(8, N, dtype=torch.float64, device="cuda").t()
    Y8 = torch.empty(8, N, dtype=torch.float64, device="cuda").t()
    # the ideal stream over arrays of the same byte mix (DESTROYS its outputs: y / Y8 scratch only)
    half = rv.view(torch.int32)[:nnz]

    def stream(inputs, outputs):
        gbs = asm.ctx.stream_mix(inputs, outputs, 2048)
        return sum(b for _, b in inputs + outputs) / (gbs * 1e9)

    mat = [(nz.data_ptr(), 8 * nnz), (half.data_ptr(), 4 * nnz)]
    s_ax = stream(mat + [(x.data_ptr(), 8 * N)], [(y.data_ptr(), 8 * N)])
    emit("A*x", timed(lambda: op.mul(x, Y=y), a.reps), 12 * nnz + 4 * N + 16 * N, s_ax, bytes_per_tracer=12 * nnz + 4 * N + 16 * N)
    s_atx = stream(mat + [(cp.data_ptr(), 8 * (N + 1)), (x.data_ptr(), 8 * N)], [(y.data_ptr(), 8 * N)])
    emit("At*x", timed(lambda: op.mul(x, Y=y, adjoint=True), a.reps), 12 * nnz + 8 * (N + 1) + 16 * N, s_atx)
    b8 = 12 * nnz + 4 * N + 8 * 8 * 2 * N
    s_8 = stream(mat + [(X8.data_ptr(), 64 * N)], [(Y8.data_ptr(), 64 * N)])
    emit("A*X k=8", timed(lambda: op.mul(X8, Y=Y8), a.reps), b8, s_8, bytes_per_tracer=b8 / 8)
    b8t = 12 * nnz + 8 * (N + 1) + 8 * 8 * 2 * N
    emit("At*X k=8", timed(lambda: op.mul(X8, Y=Y8, adjoint=True), a.reps), b8t, None, bytes_per_tracer=b8t / 8)
    # the parent's route: download T, multiply with scipy on the host
    xs = x.cpu().numpy()
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = asm.result_to_host()["T"]
        import scipy.sparse as sp

        Th = sp.csc_matrix((h[2], h[1] - 1, h[0] - 1), shape=(N, N))
        t1 = time.perf_counter()
        _ = Th @ xs
        t2 = time.perf_counter()
        host.append((t2 - t0, t1 - t0, t2 - t1))
    med = sorted(host)[1]
    lines.append({"what": "host_route (result_to_host T + scipy T @ x)", "N": N, "nnz": nnz, "total_s": med[0], "download_s": med[1], "scipy_s": med[2]})
    print(json.dumps(lines[-1]), flush=True)
    op.close()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
