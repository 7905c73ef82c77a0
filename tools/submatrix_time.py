"""Time otmb_op_submatrix_dev and otmb_op_take_values (csrc/otmb_submatrix.hip) on the 1 degree preset; one JSON line per measurement.

    python tools/submatrix_time.py [--reps 7] [--maxiter 20000] [--rtol 1e-10] [--trace] [--no-host] [--out FILE.jsonl]

The parent: T of the 1 degree preset and eleven copies scaled by 1 + 0.02·m in twelve value slots, with the water columns as lines.  The
selection: principal, the surface level dropped (the interior of the Dirichlet problem with the surface prescribed).
  submatrix   the whole call (plan, twelve slots, lines), wall time with a wait for the device, median of --reps after one warm-up;
              the twelve slot gathers alone (twelve otmb_op_take_values, HIP events) and, as the streaming yardstick, twelve
              otmb_op_set_values_slot_dev of the child from a resident nzval (a device copy plus spmv_relayout_kernel); the gather's bytes per
              launch (40 per entry of the child: src, dst and the gathered parent value read, nz and val written) against the HBM peak.
  host route  what the call replaces, on the same box: scipy indexing of twelve host matrices, otmb_op_create, eleven otmb_op_set_values
              (--no-host skips it).
  solves      the interior age problem A_II·x = 1 on the child against the restoring route (d = 1 s⁻¹ on the surface) on the parent: BiCGStab
              iterations and wall time, lines, the same rtol.
--trace: only a warm-up, twelve gathers and twelve set_values -- the run to put under a kernel trace, for the median time of sub_take_kernel
beside spmv_relayout_kernel."""
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
from otmb_amd import synthetic  # noqa: E402
from otmb_amd.device import DeviceAssembler, Operator  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X
NSLOTS = 12


def events(fn, reps):
    out = []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out[1:]


def wall(fn, reps):
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out[1:], r


def stats(t):
    return {"median_s": float(np.median(t)), "min_s": float(np.min(t)), "max_s": float(np.max(t))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--trace", action="store_true")
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
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    nsurf = int(torch.count_nonzero(asm.wet3d.view(asm.nz, -1)[0]).item())
    months = [(nz[:nnz] * (1.0 + 0.02 * m)).contiguous() for m in range(NSLOTS)]
    parent = Operator(asm.ctx, N, N, cp, rv, months[0])
    parent.set_lines(asm.vertical_lines())
    parent.set_slots(NSLOTS)
    for m in range(NSLOTS):
        parent.set_values_dev(months[m], slot=m)
    inner = torch.arange(nsurf, N, dtype=torch.int64, device="cuda")
    child = parent.submatrix(inner)
    base = {"n": N, "nnz": nnz, "child_n": child.shape[0], "child_nnz": child.nnz, "nslots": NSLOTS, "selection": "principal, surface level dropped"}
    gathered = [child.to_csc(s)[2] for s in range(NSLOTS)]

    def gathers():
        for s in range(NSLOTS):
            child.take_values(parent, slot=s)

    def scatters():
        for s in range(NSLOTS):
            child.set_values_dev(gathered[s], slot=s)

    if a.trace:
        for _ in range(3):
            gathers()
            scatters()
        torch.cuda.synchronize()
        return emit(dict(base, what="trace run: 36 sub_take_kernel and 36 spmv_relayout_kernel launches of the child's size"))

    t_sub, _ = wall(lambda: parent.submatrix(inner).close(), a.reps)
    t_g, t_s = events(gathers, a.reps), events(scatters, a.reps)
    per = float(np.median(t_g)) / NSLOTS
    moved = 40 * child.nnz
    emit(dict(base, what="submatrix", submatrix=stats(t_sub), twelve_take_values=stats(t_g), twelve_set_values_dev=stats(t_s),
              plan_estimate_s=float(np.median(t_sub) - np.median(t_g) * (NSLOTS - 1) / NSLOTS), take_values_per_launch_s=per,
              gather_bytes_per_launch=moved, gather_share_of_hbm_peak=moved / per / HBM_PEAK, reps=a.reps))

    if not a.no_host:
        import scipy.sparse as sp

        hp, hr = cp.cpu().numpy(), rv[:nnz].cpu().numpy()
        hv = [m.cpu().numpy() for m in months]
        sel = np.arange(nsurf, N)

        def host_route():
            t0 = time.perf_counter()
            subs = []
            for v in hv:
                S = sp.csc_matrix((v, hr - 1, hp - 1), shape=(N, N))[sel][:, sel]
                S.sort_indices()
                subs.append(S)
            t1 = time.perf_counter()
            S = subs[0]
            D = api.DeviceOperator(api.SparseMatrixCSC(len(sel), len(sel), S.indptr.astype(np.int64) + 1, S.indices.astype(np.int64) + 1, S.data))
            D.set_slots(NSLOTS)
            for s in range(1, NSLOTS):
                D.set_values(subs[s].data, slot=s)
            t2 = time.perf_counter()
            D.close()
            return t1 - t0, t2 - t1

        parts = [host_route() for _ in range(3)][1:]
        emit(dict(base, what="host route: scipy indexing of twelve matrices, otmb_op_create, eleven otmb_op_set_values",
                  scipy_indexing_s=float(np.median([p[0] for p in parts])), create_and_uploads_s=float(np.median([p[1] for p in parts])),
                  total_s=float(np.median([p[0] + p[1] for p in parts]))))

    ones_i = torch.ones(child.shape[0], dtype=torch.float64, device="cuda")
    ones = torch.ones(N, dtype=torch.float64, device="cuda")
    d = torch.zeros(N, dtype=torch.float64, device="cuda")
    d[:nsurf] = 1.0
    for what, op, B, dd in (("Dirichlet: A_II·x = 1 on the child", child, ones_i, None), ("restoring: (diag(d) + A)·x = 1, d = 1 on the surface", parent, ones, d)):
        t, (X, info) = wall(lambda: op.solve(B, d=dd, rtol=a.rtol, maxiter=a.maxiter, precond="lines"), min(a.reps, 3))
        emit(dict(base, what=what, precond="lines", rtol=a.rtol, iterations=int(info.iterations[0]), reason=info.reason[0], relres=float(info.relres[0]),
                  solve=stats(t)))
    child.close()
    parent.close()


if __name__ == "__main__":
    main()
