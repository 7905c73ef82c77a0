"""Times the per-column d (otmb_op_*_dk) on one GPU, one measurement per process (run it in fresh processes, alternating builds of the
library with --lib, and compare medians with the run-to-run spread of the same build: DESIGN §6 has the numbers).

    --matrix FILE.npz   colptr, rowval, nzval (Julia's arrays), nsurf and next (the water columns) of the grid, made once on the host by --make
    --what periodic3    the three-tracer example -- ideal age, radiocarbon, a dye restored over its own patch -- as ONE periodic call with the
                        n x 3 d (outer = mean, lines)
    --what periodic1x3  the same three tracers as three calls with k = 1 and a 1-D d: the only way without the per-column exports
    --what solve4       solve with k = 4 and ONE d for all columns (the existing export; --precond): what the column stride must not slow down

Every call runs on device tensors through device.Operator; a call is timed with the host clock around it after a device synchronisation
(every call here ends by reading its report, which waits for the device).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MONTH = 30 * 86400.0
LAMBDA = 1.0 / (8267.0 * 365.25 * 86400.0)  # radiocarbon: a mean life of 8267 years, in s⁻¹


def make(path):
    """The 90 x 60 x 20 grid of tests/solve_ref.py (BIG) from the CPU oracle: its T, the surface count and the water columns."""
    from oracle import oracle as orc

    import solve_lines_ref as LR

    orc.build()
    (p, i, v), N, nsurf, nxt = LR.grid(orc, "90x60x20")
    np.savez(path, colptr=p, rowval=i, nzval=v, nsurf=nsurf, next=nxt)
    print(f"{path}: N = {N}, nnz = {len(v)}, surface cells = {nsurf}")


def tracers(N, nsurf):
    """(D, S), n x 3: ideal age (restoring 1 s⁻¹ at the surface, a unit interior source), radiocarbon (the same restoring towards 1 plus λ on
    every cell), a dye restored towards 1 over the first half of the surface cells."""
    age = np.zeros(N)
    age[:nsurf] = 1.0
    patch = np.zeros(N)
    patch[:nsurf // 2] = 1.0
    D = np.asfortranarray(np.stack([age, age + LAMBDA, patch], axis=1))
    S = np.asfortranarray(np.stack([1.0 - age, age, patch], axis=1))
    return D, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", default=None)
    ap.add_argument("--make", default=None)
    ap.add_argument("--what", default="periodic3", choices=["periodic3", "periodic1x3", "solve4"])
    ap.add_argument("--precond", default="lines", choices=["jacobi", "lines"])  # of solve4
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.make:
        return make(a.make)
    import torch

    from otmb_amd import capi

    if a.lib:
        capi.use_library(a.lib, lenient=True)  # (an older build lacks the newer exports)
    from otmb_amd.device import DeviceAssembler, Operator

    import step_ref as SR

    z = np.load(a.matrix)
    p, i, v, nsurf, nxt = z["colptr"], z["rowval"], z["nzval"], int(z["nsurf"]), z["next"]
    N = len(p) - 1
    t = lambda x, dt=np.float64: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    cm = lambda x: torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()  # column-major on the device
    ctx = DeviceAssembler(0).ctx
    O = Operator(ctx, N, N, t(p, np.int64), t(i, np.int64), t(v))
    O.set_slots(3)
    for s, vals in enumerate(SR.slot_values(v, seed=1)):
        O.set_values_dev(t(vals), slot=s)
    O.set_lines(t(nxt, np.int64))
    D, S = tracers(N, nsurf)
    kw = dict(dt=MONTH, ncycle=12, theta=1.0, first_slot=0, rtol=1e-10, maxiter=5000, precond="lines", ptol=1e-8, restart=30, maxcycles=200, outer="mean")
    times, report = [], None
    for rep in range(a.reps + 1):  # the first repetition warms up (allocations, code objects) and is dropped
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.what == "periodic3":
            X, info = O.periodic(cm(S), d=cm(D), **kw)
            report = dict(cycles=info.cycles.tolist(), msolve_iters=info.msolve_iters.tolist(), converged=bool(info.converged.all()))
        elif a.what == "periodic1x3":
            infos = [O.periodic(t(S[:, c]), d=t(D[:, c]), **kw)[1] for c in range(3)]
            report = dict(cycles=[int(x.cycles[0]) for x in infos], msolve_iters=[int(x.msolve_iters[0]) for x in infos],
                          converged=all(bool(x.converged.all()) for x in infos))
        else:
            B = np.ones((N, 4), order="F")
            B[:, 1:] = np.random.default_rng(1).standard_normal((N, 3))
            X, info = O.solve(cm(B), d=t(D[:, 0]), sigma=1.0 / MONTH, rtol=1e-10, maxiter=5000, precond=a.precond)
            report = dict(precond=a.precond, iterations=info.iterations.tolist(), converged=bool(info.converged.all()))
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    print(json.dumps(dict(what=a.what, lib=a.lib or "this build", N=N, seconds=times, median=float(np.median(times)), **report)))


if __name__ == "__main__":
    main()
