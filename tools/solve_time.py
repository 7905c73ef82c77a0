"""Time the device solver (otmb_op_solve_pc_dev, csrc/otmb_solve.hip) on the 1 degree preset; one JSON line per measurement.

    python tools/solve_time.py [--reps 10] [--maxiter 20000] [--precond jacobi|lines|both] [--year] [--host] [--out FILE.jsonl]

Systems (B = 1, rtol = 1e-10):
    age      d = 1 s⁻¹ on the level-1 wet cells, σ = 0, on the full T and on the 2 x 2 x 1 coarse operator LUMP * T * SPRAY with
             d_c = (LUMP * issrf .> 0), b_c = LUMP * 1 (the reference's own case, test/local_full.jl:151-188)
    month    σ = 1 / (30 d), d = 0, on T
    year     σ = 1 / (365 d), d = 0, on T (--year; with Jacobi it runs into --maxiter)
--precond: the preconditioner(s) to time.  lines: the water columns (DeviceAssembler.vertical_lines) on T; on the coarse operator the
    fine columns seen through LUMP (a coarse cell's successor is the coarse cell of a fine successor: the first such pair per cell, and per
    successor -- an ARBITRARY choice among the candidates, not a tuned coarse preconditioner: the record says so in lines_note).
    A lines record also has setup_plus_one_sweep_us: one otmb_op_precond_dev call with k = 1, i.e. diagonal, extraction, factorisation, ONE
    sweep and one wait for the device -- an upper bound of the extraction plus factorisation a solve pays once; with --precond both the
    line after it estimates the sweep as half the difference of the two per-iteration times and subtracts it (setup_estimate_us).
Each line: iterations, reason, relres, the median / min / max wall time of --reps solves after one warm-up (time.perf_counter around the
call, which waits for the device), the time per iteration, and the time of two otmb_op_mul_dev products on the same operator (HIP events):
the floor of an iteration, whose five vector passes and scalar kernels the fusion is to keep small.
--step [--step-route step|compose|both]: the time loop instead of the solves above -- T of the 1 degree preset and eleven copies of it
    scaled by 1 + 0.02·m as twelve monthly matrices, k = 1, precond = lines, θ = 1, δt = 30 d, 24 steps (two years) from X = 1, the median
    of --reps after one warm-up.  Route `step`: the twelve matrices in value slots, ONE otmb_op_step_dev call.  Route `compose`: the same
    24 steps in the public device calls there were before the slots -- otmb_op_set_values_dev of the month's values, the right-hand side
    σ·x as a torch operation, otmb_op_solve_pc_dev from x -- which is what runs against a library of an earlier commit as well (it uses
    no newer symbol: --lib PATH loads another build of the library, an earlier commit's for the baseline).  The solve is called in place on
    one X (no allocation or copy per step that the step call would not make either).  The record also times, around this process's calls:
    a slot's first visit as otmb_op_precond_dev (setup plus one sweep and one wait, the upper bound of above), one solve with its setup, one
    step call of one step, and from these a later visit (right-hand side plus solve).  rhs_torch_us is the COMPOSITION's right-hand side,
    torch's σ·x (HIP events around 24 of them); the step call's own right-hand-side kernel has no entry point to time it through and is
    read from a kernel trace of `--step --step-route step` instead.  The record carries the device memory the slots take.
--step --substeps M: M implicit steps inside every one of the twelve months, the age system -- ONE otmb_op_step_sched_dev call against the same
    12·M steps as one-step otmb_op_step_dev calls, alternating in one process (substeps_times).
--step --interp: the TMM convention on that year -- twelve slots, `lines`, θ = 1, the age system, k = 1, four sub-steps a month, the schedule
    of api.interp_schedule(12, 4): 48 steps, every one blended.  Route `interp`: ONE otmb_op_step_interp_dev call.  Route `chain`: the same 48
    steps in the public calls there were before it -- otmb_op_combine_slots_dev into a thirteenth slot, then a one-step otmb_op_step_dev on
    it -- which is what runs against an earlier commit's library as well (--lib PATH: only `chain` runs then).  Medians of 7 after one
    warm-up of each (interp_times); the record also times one blend by otmb_op_combine_slots_dev (HIP events) and a preconditioner's setup
    plus one sweep and one wait (otmb_op_precond_dev), the upper bound of what every blended step pays.
--season: the same 48 blended steps with d and the source per slot -- the age d and a unit source, each scaled by a monthly factor (an ice
    cover).  Route `season`: ONE otmb_op_step_season_dev call.  Route `chain`: otmb_op_combine_slots_dev into a thirteenth slot, d_t and s_t
    blended by tensor operations, then a one-step otmb_op_step_dev -- public calls of the commits before it, so it runs against an earlier
    library as well (--lib PATH: only `chain` runs then).  Medians of 7 after one warm-up of each, the routes alternating, the states
    compared bit for bit (season_times).  The fold kernel's own time is read from a kernel trace of this run; at k = 1 it moves
    3·8·n bytes a launch, which is a launch-bound size.
--periodic [--outer none|mean --ptol --restart --maxcycles --rtol]: the periodic state of that year -- the twelve slots of --step, θ = 1, lines, the age system
    (d = 1 s⁻¹ at the surface, s = 1), k = 1 -- by otmb_op_periodic_dev: cycles, wall time, defect; then, in the same process, the same
    number of plain cycles by otmb_op_step_dev in a loop from zero: their wall time and the defect they leave.  --outer mean: the outer GMRES
    preconditioned by the cycle-mean operator (otmb_op_periodic_pc_dev); the record then carries the mean solves' iterations and the wall time
    of one mean solve (the twelve slots' mean by otmb_op_combine_slots_dev in a thirteenth slot, σ = 0, from zero) beside that of one cycle.
    --outer none is the call of the commits before the keyword.
--host: the parent's only route as well -- result_to_host, then scipy.sparse.linalg.bicgstab with the same (Jacobi) preconditioner."""
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

DAY = 86400.0


def two_products(op, n, reps=30):
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    for _ in range(5):
        op.mul(x, Y=y)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        op.mul(x, Y=y)
        op.mul(y, Y=x)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(out))


def step_times(asm, a):
    nslots, nsteps, dt = 12, 24, 30 * DAY
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    months = [(nz[:nnz] * (1.0 + 0.02 * m)).contiguous() for m in range(nslots)]
    nxt = asm.vertical_lines()
    x0 = torch.ones(N, dtype=torch.float64, device="cuda")
    sigma = 1.0 / (1.0 * dt)
    routes = ["step", "compose"] if a.step_route == "both" else [a.step_route]
    recs = []
    for route in routes:
        free0 = torch.cuda.mem_get_info()[0]
        op = Operator(asm.ctx, N, N, cp, rv, months[0])
        op.set_lines(nxt)
        rec = {"what": "24 monthly steps, T", "route": route, "n": N, "nnz": nnz, "nslots": nslots, "nsteps": nsteps, "precond": "lines",
               "theta": 1.0, "dt_s": dt, "reps": a.reps}
        if route == "step":
            torch.cuda.synchronize()
            free1 = torch.cuda.mem_get_info()[0]
            op.set_slots(nslots)
            for m in range(nslots):
                op.set_values_dev(months[m], slot=m)
            torch.cuda.synchronize()
            rec["slots_bytes"] = int(free1 - torch.cuda.mem_get_info()[0])  # the eleven slots beyond the operator's own
            rec["slot_bytes_exact"] = 8 * nnz  # + 8 x (the row layout's entries, padding included), per slot
        times, its = [], None
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "step":
                X, info = op.step(x0, dt=dt, theta=1.0, nsteps=nsteps, first_slot=0, rtol=1e-10, maxiter=a.maxiter, precond="lines")
                its = info.iterations[:, 0].tolist()
                assert info.steps_done == nsteps, info
            else:
                X, B, its = x0.clone(), torch.empty_like(x0), []
                it1, rr1, why1 = np.zeros(1, dtype=np.int64), np.zeros(1), np.zeros(1, dtype=np.int32)
                for t in range(nsteps):
                    op.set_values_dev(months[t % nslots])
                    torch.mul(X, sigma, out=B)
                    rc = op.lib.otmb_op_solve_pc_dev(op.handle, 0, 1, None, sigma, B.data_ptr(), N, X.data_ptr(), N, 1, 1e-10, a.maxiter,
                                                     it1.ctypes.data, rr1.ctypes.data, why1.ctypes.data, 1)  # in place, from X, "lines"
                    assert rc == 0, (rc, t, int(why1[0]))
                    its.append(int(it1[0]))
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        times = times[1:]
        rec.update(iterations=its, median_s=float(np.median(times)), min_s=float(np.min(times)), max_s=float(np.max(times)),
                   per_step_us=float(np.median(times)) / nsteps * 1e6, checksum=float(X.sum().item()))
        # the parts of a step that calls of this process can bracket: the composition's right-hand side (torch's), a slot's first visit, a solve
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(nsteps):
            B = sigma * x0
        ev[1].record()
        ev[1].synchronize()
        rec["rhs_torch_us"] = ev[0].elapsed_time(ev[1]) * 1e3 / nsteps
        tp = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op.precondition(x0, sigma=sigma)
            torch.cuda.synchronize()
            tp.append(time.perf_counter() - t0)
        rec["first_visit_upper_bound_us"] = float(np.median(tp[1:])) * 1e6  # setup + one sweep + one wait
        ts = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op.solve(sigma * x0, sigma=sigma, rtol=1e-10, maxiter=a.maxiter, x0=x0, precond="lines")
            ts.append(time.perf_counter() - t0)
        rec["one_solve_us"] = float(np.median(ts[1:])) * 1e6  # setup included, as the composition pays it
        if route == "step":
            ts1 = []
            for r in range(a.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                op.step(x0, dt=dt, nsteps=1, rtol=1e-10, maxiter=a.maxiter, precond="lines")
                ts1.append(time.perf_counter() - t0)
            rec["one_step_call_us"] = float(np.median(ts1[1:])) * 1e6  # first visit + right-hand side + solve
            rec["later_visit_us"] = (rec["median_s"] * 1e6 - nslots * rec["one_step_call_us"]) / (nsteps - nslots)  # right-hand side + solve
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        op.close()
        del op
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


def substeps_times(asm, a):
    """--step --substeps M: the twelve months of --step as value slots, θ = 1, `lines`, the age system (d = 1 s⁻¹ on the level-1 wet cells,
    s = 1), k = 1, M implicit steps of δt = 30 d / M inside every month: 12·M steps from zero.  Route `sched`: ONE otmb_op_step_sched_dev call
    (one preconditioner per slot, no wait per step).  Route `loop`: the same 12·M steps as 12·M one-step otmb_op_step_dev calls, what the
    interface offered before the schedule (a fresh preconditioner and a host round trip per sub-step).  Both in this process with this
    library, alternating, the median of --reps (at least 5) after one warm-up of each; the two routes' states are compared bit for bit."""
    nslots, m = 12, int(a.substeps)
    nsteps, dt = nslots * m, 30 * DAY / m
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    op = Operator(asm.ctx, N, N, cp, rv, (nz[:nnz] * 1.0).contiguous())
    op.set_lines(asm.vertical_lines())
    op.set_slots(nslots)
    for s in range(nslots):
        op.set_values_dev((nz[:nnz] * (1.0 + 0.02 * s)).contiguous(), slot=s)
    nsurf = int(torch.count_nonzero(asm.wet3d.reshape(-1)[: asm.nx * asm.ny]).item())
    d = torch.zeros(N, dtype=torch.float64, device="cuda")
    d[:nsurf] = 1.0
    src, x0 = torch.ones(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
    kw = dict(dt=dt, theta=1.0, source=src, d=d, rtol=a.rtol, maxiter=a.maxiter, precond="lines")

    def sched():
        X, info = op.step_sched(x0, nsteps=nsteps, first_slot=0, substeps=m, **kw)
        assert info.steps_done == nsteps, info
        return X, int(info.iterations.sum())

    def loop():
        X, its = x0, 0
        for t in range(nsteps):
            X, info = op.step(X, nsteps=1, first_slot=(t // m) % nslots, **kw)
            assert info.steps_done == 1, (t, info)
            its += int(info.iterations.sum())
        return X, its

    times, out = {"sched": [], "loop": []}, {}
    for r in range(max(a.reps, 5) + 1):
        for name, route in (("sched", sched), ("loop", loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = route()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    rec = {"what": "12 months x M implicit sub-steps, T, age system", "n": N, "nnz": nnz, "nslots": nslots, "substeps": m, "nsteps": nsteps, "precond": "lines",
           "theta": 1.0, "dt_s": dt, "reps": max(a.reps, 5), "iterations": out["sched"][1], "loop_iterations": out["loop"][1],
           "same_bits": bool(torch.equal(out["sched"][0], out["loop"][0])), "checksum": float(out["sched"][0].sum().item())}
    for name in times:
        t = times[name][1:]
        rec.update({name + "_median_s": float(np.median(t)), name + "_min_s": float(np.min(t)), name + "_max_s": float(np.max(t))})
    print(json.dumps(rec), flush=True)
    op.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


def season_times(asm, a):
    """--season: see the module's text.  The two routes' states are compared bit for bit when both run."""
    nslots, m, reps = 12, 4, 7
    nsteps, dt = nslots * m, 30 * DAY / m
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    op = Operator(asm.ctx, N, N, cp, rv, (nz[:nnz] * 1.0).contiguous())
    op.set_lines(asm.vertical_lines())
    op.set_slots(nslots + 1)  # the thirteenth: the chain's scratch
    for s in range(nslots):
        op.set_values_dev((nz[:nnz] * (1.0 + 0.02 * s)).contiguous(), slot=s)
    nsurf = int(torch.count_nonzero(asm.wet3d.reshape(-1)[: asm.nx * asm.ny]).item())
    d = torch.zeros(N, dtype=torch.float64, device="cuda")
    d[:nsurf] = 1.0
    ice = [0.55 + 0.45 * float(np.cos(2.0 * np.pi * s / nslots)) for s in range(nslots)]  # the monthly factor 1 - ice, in 0.1 .. 1
    spare = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")  # the scratch slot's block: no step names it
    ds = [(d * f).contiguous() for f in ice] + [spare]
    ss = [torch.full((N,), f, dtype=torch.float64, device="cuda") for f in ice] + [spare]
    x0 = torch.zeros(N, dtype=torch.float64, device="cuda")
    kw = dict(dt=dt, theta=1.0, rtol=a.rtol, maxiter=a.maxiter, precond="lines")
    sa, sb, w = api.interp_schedule(nslots, m)
    assert len(w) == nsteps and ((w > 0) & (w < 1)).all()

    def season():
        X, info = op.step_season(x0, slot_a=sa, slot_b=sb, weight=w, d=ds, source=ss, **kw)
        assert info.steps_done == nsteps, info
        return X, int(info.iterations.sum())

    def chain():
        X, its = x0, 0
        for t in range(nsteps):
            wa, wb = 1.0 - float(w[t]), float(w[t])
            wt = np.zeros(nslots + 1)
            wt[sa[t]], wt[sb[t]] = wa, wb
            op.combine_slots(wt, nslots)
            dt_ = wa * ds[sa[t]] + wb * ds[sb[t]]  # (two products and a sum, each rounded: tensor operations do not contract)
            st = wa * ss[sa[t]] + wb * ss[sb[t]]
            X, info = op.step(X, nsteps=1, first_slot=nslots, d=dt_, source=st, **kw)
            assert info.steps_done == 1, (t, info)
            its += int(info.iterations.sum())
        return X, its

    routes = [("chain", chain)] + ([("season", season)] if hasattr(op.lib, "otmb_op_step_season_dev") else [])
    times, out = {name: [] for name, _ in routes}, {}
    for r in range(reps + 1):
        for name, route in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = route()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    rec = {"what": "12 months x 4 sub-steps, TMM interpolation, T, age d and unit source scaled by a monthly factor", "n": N, "nnz": nnz, "nslots": nslots,
           "substeps": m, "nsteps": nsteps, "precond": "lines", "theta": 1.0, "dt_s": dt, "reps": reps, "lib": a.lib or "this build",
           "fold_bytes": 3 * 8 * N, "fold_launches": 2 * nsteps, "iterations": out["chain"][1], "checksum": float(out["chain"][0].sum().item())}
    if "season" in out:
        rec.update(season_iterations=out["season"][1], same_bits=bool(torch.equal(out["season"][0], out["chain"][0])))
    for name in times:
        t = times[name][1:]
        rec.update({name + "_median_s": float(np.median(t)), name + "_min_s": float(np.min(t)), name + "_max_s": float(np.max(t))})
    print(json.dumps(rec), flush=True)
    op.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


def interp_times(asm, a):
    """--step --interp: see the module's text.  The two routes' states are compared bit for bit when both run."""
    nslots, m, reps = 12, 4, 7
    nsteps, dt = nslots * m, 30 * DAY / m
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    op = Operator(asm.ctx, N, N, cp, rv, (nz[:nnz] * 1.0).contiguous())
    op.set_lines(asm.vertical_lines())
    op.set_slots(nslots + 1)  # the thirteenth: the chain's scratch
    for s in range(nslots):
        op.set_values_dev((nz[:nnz] * (1.0 + 0.02 * s)).contiguous(), slot=s)
    nsurf = int(torch.count_nonzero(asm.wet3d.reshape(-1)[: asm.nx * asm.ny]).item())
    d = torch.zeros(N, dtype=torch.float64, device="cuda")
    d[:nsurf] = 1.0
    src, x0 = torch.ones(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
    kw = dict(dt=dt, theta=1.0, source=src, d=d, rtol=a.rtol, maxiter=a.maxiter, precond="lines")
    sa, sb, w = api.interp_schedule(nslots, m)
    assert len(w) == nsteps and ((w > 0) & (w < 1)).all()

    def interp():
        X, info = op.step_interp(x0, slot_a=sa, slot_b=sb, weight=w, **kw)
        assert info.steps_done == nsteps, info
        return X, int(info.iterations.sum())

    def chain():
        X, its = x0, 0
        for t in range(nsteps):
            wt = np.zeros(nslots + 1)
            wt[sa[t]], wt[sb[t]] = 1.0 - float(w[t]), float(w[t])
            op.combine_slots(wt, nslots)
            X, info = op.step(X, nsteps=1, first_slot=nslots, **kw)
            assert info.steps_done == 1, (t, info)
            its += int(info.iterations.sum())
        return X, its

    # the row layout's entries, padding included, by the plan's rule (csrc/otmb_spmv.hip): slices of 64 rows as wide as their longest short row,
    # the long rows (more than 256 entries, or more than 32 and four times the slice's mean) behind them
    lens = torch.bincount(rv[:nnz] - 1, minlength=N).cpu().numpy().astype(np.int64)
    L = np.zeros(-(-N // 64) * 64, dtype=np.int64)
    L[:N] = lens
    L = L.reshape(-1, 64)
    rows = np.minimum(64, N - 64 * np.arange(len(L)))
    mean = -(-L.sum(axis=1) // np.maximum(rows, 1))
    lng = (L > 256) | ((L > 32) & (L > 4 * mean[:, None]))
    nval = int(64 * np.where(lng, 0, L).max(axis=1).sum() + L[lng].sum())
    routes = [("chain", chain)] + ([("interp", interp)] if hasattr(op.lib, "otmb_op_step_interp_dev") else [])
    times, out = {name: [] for name, _ in routes}, {}
    for r in range(reps + 1):
        for name, route in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = route()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    rec = {"what": "12 months x 4 sub-steps, TMM interpolation, T, age system", "n": N, "nnz": nnz, "nslots": nslots, "substeps": m, "nsteps": nsteps,
           "precond": "lines", "theta": 1.0, "dt_s": dt, "reps": reps, "lib": a.lib or "this build", "nval": nval, "blend_bytes": 24 * (nnz + nval), "iterations": out["chain"][1],
           "checksum": float(out["chain"][0].sum().item())}
    if "interp" in out:
        rec.update(interp_iterations=out["interp"][1], same_bits=bool(torch.equal(out["interp"][0], out["chain"][0])))
    for name in times:
        t = times[name][1:]
        rec.update({name + "_median_s": float(np.median(t)), name + "_min_s": float(np.min(t)), name + "_max_s": float(np.max(t))})
    # one blend through the public combine (two launches), and a preconditioner's setup + one sweep + one wait on the blended values
    wt = np.zeros(nslots + 1)
    wt[0], wt[1] = 0.375, 0.625
    ev = []
    for r in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        op.combine_slots(wt, nslots)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    rec["combine_slots_event_s"] = float(np.median(ev[2:]))
    op.select(nslots)
    ts = []
    for r in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.precondition(src, d=d, sigma=1.0 / dt, precond="lines")
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    op.select(0)
    rec["setup_plus_one_sweep_s"] = float(np.median(ts[1:]))
    print(json.dumps(rec), flush=True)
    op.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


def periodic_times(asm, a):
    """--periodic: the twelve months of --step as value slots, θ = 1, δt = 30 d, `lines`, the age system (d = 1 s⁻¹ on the level-1 wet cells,
    s = 1), k = 1: the periodic state by otmb_op_periodic_dev (GMRES(--restart) on the cycle of twelve steps, to --ptol, at most --maxcycles
    cycles), its cycles and wall time, and -- in the same process, with the same library -- the same number of plain cycles by
    otmb_op_step_dev called in a loop from zero, their wall time and the defect ‖F(x) - x‖₂/‖F(0)‖₂ they leave."""
    nslots, dt = 12, 30 * DAY
    N = asm.N
    cp, rv, nz = asm.out["T"]
    nnz = int(cp[N].item()) - 1
    op = Operator(asm.ctx, N, N, cp, rv, (nz[:nnz] * 1.0).contiguous())
    op.set_lines(asm.vertical_lines())
    op.set_slots(nslots)
    for m in range(nslots):
        op.set_values_dev((nz[:nnz] * (1.0 + 0.02 * m)).contiguous(), slot=m)
    nsurf = int(torch.count_nonzero(asm.wet3d.reshape(-1)[: asm.nx * asm.ny]).item())  # level 1 comes first, in the grid and among the wet cells
    d = torch.zeros(N, dtype=torch.float64, device="cuda")
    d[:nsurf] = 1.0
    s = torch.ones(N, dtype=torch.float64, device="cuda")
    kw = dict(dt=dt, theta=1.0, first_slot=0, d=d, rtol=a.rtol, maxiter=a.maxiter, precond="lines")
    rec = {"what": "periodic state of twelve monthly steps, T, age system", "n": N, "nnz": nnz, "nslots": nslots, "ncycle": nslots, "precond": "lines",
           "theta": 1.0, "dt_s": dt, "ptol": a.ptol, "restart": a.restart, "maxcycles": a.maxcycles, "rtol": a.rtol, "outer": a.outer}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    X, info = op.periodic(s, ncycle=nslots, ptol=a.ptol, restart=a.restart, maxcycles=a.maxcycles, outer=a.outer, **kw)
    torch.cuda.synchronize()
    rec.update(periodic_s=time.perf_counter() - t0, cycles=int(info.cycles[0]), defect=float(info.defect[0]), reason=info.reason[0],
               msolve_iters=int(info.msolve_iters[0]), checksum=float(X.sum().item()))
    # the same number of plain cycles from zero, then one more to measure what they leave
    G, si = op.step(torch.zeros_like(s), nsteps=nslots, source=s, **kw)
    assert si.steps_done == nslots, si
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Y = torch.zeros_like(s)
    for _ in range(rec["cycles"]):
        Y, si = op.step(Y, nsteps=nslots, source=s, **kw)
        assert si.steps_done == nslots, si
    torch.cuda.synchronize()
    rec["plain_s"] = time.perf_counter() - t0
    FY, si = op.step(Y, nsteps=nslots, source=s, **kw)
    rec["plain_defect"] = float((torch.linalg.norm(FY - Y) / torch.linalg.norm(G)).item())
    rec["per_cycle_s"] = rec["plain_s"] / max(rec["cycles"], 1)
    if a.outer == "mean":  # one mean solve on its own: the right-hand side a unit vector, as a basis vector is
        op.set_slots(nslots + 1)
        op.combine_slots([1.0 / nslots] * nslots + [0.0], nslots)
        op.select(nslots)
        v = s / torch.linalg.norm(s)
        ts = []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, mi = op.solve(v, d=d, sigma=0.0, rtol=a.rtol, maxiter=a.maxiter, precond="lines")
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rec.update(mean_solve_s=float(np.median(ts[1:])), mean_solve_iters=int(mi.iterations[0]), mean_solve_reason=mi.reason[0])
    print(json.dumps(rec), flush=True)
    op.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--precond", default="jacobi", choices=["jacobi", "lines", "both"])
    ap.add_argument("--year", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--step-route", default="both", choices=["step", "compose", "both"])
    ap.add_argument("--substeps", type=int, default=0)
    ap.add_argument("--interp", action="store_true")
    ap.add_argument("--season", action="store_true")
    ap.add_argument("--periodic", action="store_true")
    ap.add_argument("--outer", default="none", choices=["none", "mean"])
    ap.add_argument("--ptol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--maxcycles", type=int, default=200)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        from otmb_amd import capi

        capi.use_library(os.path.abspath(a.lib), lenient=True)
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    g = synthetic.preset("access1deg", rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    N = asm.N
    if a.season:
        return season_times(asm, a)
    if a.step and a.interp:
        return interp_times(asm, a)
    if a.step and a.substeps > 0:
        return substeps_times(asm, a)
    if a.step:
        return step_times(asm, a)
    if a.periodic:
        return periodic_times(asm, a)
    t0 = time.perf_counter()
    h = asm.result_to_host()["T"]
    t_download = time.perf_counter() - t0
    wet = asm.wet3d.cpu().numpy().reshape(g.umo.data.shape, order="F") != 0
    nsurf = int(np.count_nonzero(wet[:, :, 0]))
    issrf = np.zeros(N)
    issrf[:nsurf] = 1.0
    T = api.SparseMatrixCSC(N, N, *h)
    vol = np.asarray(gm.v3D).reshape(-1, order="F")[wet.reshape(-1, order="F")]
    L, S, vc = api.lump_and_spray(wet, vol, T, None, di=2, dj=2, dk=1)
    Nc = len(vc)
    L = api.SparseMatrixCSC(Nc, N, L.colptr, L.rowval, L.nzval)
    S = api.SparseMatrixCSC(N, Nc, S.colptr, S.rowval, S.nzval)
    Tc = api.coarsen(L, T, S)
    Ls = sp.csc_matrix((L.nzval, L.rowval - 1, L.colptr - 1), shape=(Nc, N))
    nxt = asm.vertical_lines()
    # the coarse operator's lines: the fine columns through LUMP (one entry per column of LUMP: rowval = the coarse cell of a fine cell)
    fine = nxt.cpu().numpy()
    i = np.flatnonzero(fine)
    ci, cj = L.rowval[i], L.rowval[fine[i] - 1]
    keep = cj > ci
    ci, cj = ci[keep], cj[keep]
    order = np.lexsort((cj, ci))
    ci, cj = ci[order], cj[order]
    first = np.r_[True, ci[1:] != ci[:-1]]  # one successor per coarse cell
    ci, cj = ci[first], cj[first]
    order = np.lexsort((ci, cj))
    ci, cj = ci[order], cj[order]
    first = np.r_[True, cj[1:] != cj[:-1]]  # nobody is the successor of two
    nxt_c = np.zeros(Nc, dtype=np.int64)
    nxt_c[ci[first] - 1] = cj[first]
    cases = [("age, coarse 2x2x1", Tc, Nc, (Ls @ issrf > 0).astype(np.float64), 0.0, Ls @ np.ones(N), torch.from_numpy(nxt_c).cuda()),
             ("age, T", T, N, issrf, 0.0, np.ones(N), nxt),
             ("month, T", T, N, None, 1.0 / (30 * DAY), np.ones(N), nxt)]
    if a.year:
        cases.append(("year, T", T, N, None, 1.0 / (365 * DAY), np.ones(N), nxt))
    preconds = ["jacobi", "lines"] if a.precond == "both" else [a.precond]
    lines = []
    for (what, A, n, d, sigma, b, nx), precond in ((c, p) for c in cases for p in preconds):
        cp, rv, nz = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (A.colptr, A.rowval, A.nzval))
        op = Operator(asm.ctx, n, n, cp, rv, nz)
        bd = torch.from_numpy(b).cuda()
        dd = None if d is None else torch.from_numpy(d).cuda()
        if precond == "lines":
            op.set_lines(nx)
        times = []
        for rep in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X, info = op.solve(bd, d=dd, sigma=sigma, rtol=1e-10, maxiter=a.maxiter, precond=precond)
            times.append(time.perf_counter() - t0)
        times = times[1:]
        its = int(info.iterations[0])
        rec = {"what": what, "precond": precond, "n": n, "nnz": int(op.nnz), "iterations": its, "reason": info.reason[0],
               "relres": float(info.relres[0]),
               "median_s": float(np.median(times)), "min_s": float(np.min(times)), "max_s": float(np.max(times)), "reps": a.reps,
               "per_iteration_us": float(np.median(times)) / max(its, 1) * 1e6, "two_products_us": two_products(op, n) * 1e6}
        if precond == "lines":
            tp = []
            for rep in range(a.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                op.precondition(bd, d=dd, sigma=sigma)
                torch.cuda.synchronize()
                tp.append(time.perf_counter() - t0)
            links = int(np.count_nonzero(nx.cpu().numpy()))
            rec.update(lines=n - links, links=links, setup_plus_one_sweep_us=float(np.median(tp[1:])) * 1e6)
            if nx is not nxt:
                rec["lines_note"] = "coarse lines: the fine water columns through LUMP, the first successor per coarse cell (arbitrary)"
            jac = [r for r in lines if r["what"] == what and r["precond"] == "jacobi"]
            if jac:
                sweep = (rec["per_iteration_us"] - jac[0]["per_iteration_us"]) / 2
                rec.update(sweep_estimate_us=sweep, setup_estimate_us=rec["setup_plus_one_sweep_us"] - sweep)
        if a.host:
            t0 = time.perf_counter()
            M = (sp.diags(np.full(n, sigma) + (0.0 if d is None else d)) + sp.csc_matrix((A.nzval, A.rowval - 1, A.colptr - 1), shape=(n, n))).tocsr()
            dg = M.diagonal()
            count = [0]

            def cb(_):
                count[0] += 1

            xh, flag = spla.bicgstab(M, b, rtol=1e-10, atol=0.0, maxiter=a.maxiter, M=spla.LinearOperator((n, n), matvec=lambda z: z / dg), callback=cb)
            t_host = time.perf_counter() - t0
            rec.update(host_scipy_s=t_host, host_download_s=t_download if A is T else 0.0, host_iterations=count[0], host_flag=int(flag),
                       host_relres=float(np.linalg.norm(b - M @ xh) / np.linalg.norm(b)))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        op.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
