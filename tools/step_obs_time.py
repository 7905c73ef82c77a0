"""Time the observed step (otmb_op_step_obs_dev, csrc/otmb_step.hip and csrc/otmb_observe.hip) on the 1 degree preset; one JSON line per route.

    python tools/step_obs_time.py [--reps 7] [--routes step,obs0,record,single,pass] [--lib PATH] [--out FILE.jsonl]

The year of tools/solve_time.py --step: T of the preset and eleven copies scaled by 1 + 0.02·m in twelve value slots, k = 1, precond = lines,
θ = 1, δt = 30 d, nsteps = 12 from X = 1.  Every time is a host clock around a call that ends in a device synchronise, the median / min / max of
--reps after one warm-up.
    step    ONE otmb_op_step_dev call (device.Operator.step).  With --lib PATH this runs against another build of the library -- an earlier
            commit's, for the baseline: it uses no newer symbol.
    obs0    otmb_op_step_obs_dev with q = 0 and no mean: the same loop and kernels as `step`.
    record  ONE call with q = 1 (W = the cell volumes: the inventory) and the mean with weights 1/12.
    single  the only route to the same outputs without the call: twelve nsteps = 1 calls of step, each followed by a download of the state and
            numpy's dot product and mean update on the host.  (Through the device route, so X, S and d are not staged again per call as the
            host entry point would; the slot's preconditioner is recomputed per call either way.)
    pass    `observe` alone (q = 1, k = 1: reads W and X, 16 B a row), HIP events around 50 calls: kernel, fold and the result's allocation.
            The pass with the mean (reads W, X and Xbar, writes Xbar: 32 B a row) runs only inside a step call; it is read from a kernel
            trace of `--routes record` (ob_kernel and ob_fold_kernel beside st_stream_kernel, which reads X and writes B: 16 B a row, in
            the same process)."""
import argparse
import ctypes as C
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

DAY = 86400.0
NSLOTS = NSTEPS = 12
DT = 30 * DAY


def timed(reps, call):
    times, out = [], None
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times = times[1:]
    return out, {"median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "times_s": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--routes", default="step,obs0,record,single,pass")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.lib:
        from otmb_amd import capi

        capi.use_library(os.path.abspath(a.lib), lenient=True)
    g = synthetic.preset("access1deg", rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    op = Operator(asm.ctx, N, N, cp, rv, nz[:nnz].contiguous())
    op.set_lines(asm.vertical_lines())
    op.set_slots(NSLOTS)
    for m in range(NSLOTS):
        op.set_values_dev((nz[:nnz] * (1.0 + 0.02 * m)).contiguous(), slot=m)
    wet = asm.wet3d.cpu().numpy().reshape(g.umo.data.shape, order="F") != 0
    vol = np.ascontiguousarray(np.asarray(gm.v3D).reshape(-1, order="F")[wet.reshape(-1, order="F")], dtype=np.float64)
    W = torch.from_numpy(vol).cuda()
    x0 = torch.ones(N, dtype=torch.float64, device="cuda")
    tw = np.full(NSTEPS, 1.0 / NSTEPS)
    kw = dict(dt=DT, theta=1.0, rtol=1e-10, maxiter=a.maxiter, precond="lines")
    base = {"n": N, "nnz": nnz, "nslots": NSLOTS, "nsteps": NSTEPS, "precond": "lines", "theta": 1.0, "dt_s": DT, "reps": a.reps, "tag": a.tag,
            "lib": a.lib}
    recs = []

    def emit(route, **more):
        rec = dict(base, route=route, **more)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for route in a.routes.split(","):
        if route == "step":
            (X, info), t = timed(a.reps, lambda: op.step(x0, nsteps=NSTEPS, first_slot=0, **kw))
            assert info.steps_done == NSTEPS, info
            emit(route, iterations=info.iterations[:, 0].tolist(), checksum=float(X.sum().item()), **t)
        elif route == "obs0":
            from otmb_amd.api import step_arrays

            def call():
                X = x0.clone()
                iters, relres, reason = step_arrays(NSTEPS, 1)
                done = C.c_int64(0)
                rc = op.lib.otmb_op_step_obs_dev(op.handle, 0, 1, None, DT, 1.0, NSTEPS, 0, None, N, X.data_ptr(), N, 1e-10, a.maxiter, 1, C.byref(done),
                                                 iters.ctypes.data, relres.ctypes.data, reason.ctypes.data, 0, None, N, None, None, None, N)
                assert rc == 0 and done.value == NSTEPS, (rc, done.value)
                return X, iters

            (X, iters), t = timed(a.reps, call)
            emit(route, iterations=iters[:, 0].tolist(), checksum=float(X.sum().item()), **t)
        elif route == "record":
            (X, info), t = timed(a.reps, lambda: op.step(x0, nsteps=NSTEPS, first_slot=0, observe=W, time_weights=tw, **kw))
            assert info.steps_done == NSTEPS, info
            emit(route, iterations=info.iterations[:, 0].tolist(), checksum=float(X.sum().item()),
                 inventory=info.observations[:, 0, 0].cpu().numpy().tolist(), mean_checksum=float(info.mean.sum().item()), **t)
        elif route == "single":
            def call():
                X, inv, mean = x0, [], np.zeros(N)
                for s in range(NSTEPS):
                    X, info = op.step(X, nsteps=1, first_slot=s % NSLOTS, **kw)
                    assert info.steps_done == 1, info
                    xh = X.cpu().numpy()
                    inv.append(float(vol @ xh))
                    mean += tw[s] * xh
                return X, inv, mean

            (X, inv, mean), t = timed(a.reps, call)
            emit(route, checksum=float(X.sum().item()), inventory=inv, mean_checksum=float(mean.sum()), **t)
        elif route == "pass":
            for _ in range(5):
                op.observe(W, x0)
            torch.cuda.synchronize()
            out = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(50):
                    op.observe(W, x0)
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e-3 / 50)
            med = float(np.median(out))
            emit(route, what="observe, q = 1, k = 1 (kernel + fold + the result's allocation)", median_s=med, min_s=float(np.min(out)), max_s=float(np.max(out)),
                 bytes=16 * N, gbytes_per_s=16 * N / med * 1e-9)
        else:
            raise SystemExit(f"unknown route {route!r}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
