#!/usr/bin/env python3
"""bench.py -- wet-cells/s assembled into T on the synthetic ACCESS-ESM1-5-like 1° grid.

One "step" = one pass of the hot path over one (umo, vmo) field, all device resident:
    facefluxesfrommasstransport -> transportmatrix (T, Tadv, TκH, TκVML, TκVdeep in CSC)
Inputs are in HBM before the timed region starts and the five CSC matrices are left in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload access1deg|quarterdeg|tenthdeg|small]
                    [--scaling weak|strong] [--repeats R] [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times EXACTLY K steps once and prints the headline line.  --full adds everything else the line
can carry: per-kernel times and the roofline, the fused and given-operator steps, the other configurations (fresh processes),
end_to_end, cpu_baseline, config2, box_probe, the communicator figures and config4 -- and repeats the K steps R = 5 times.
--dump-outputs DIR: after the timed steps, the last step's matrices and face fluxes (a fixed, seeded sample) as DIR/<name>.npy.

N > 1: one rank per GPU.  Launched by torch.distributed.run (RANK/LOCAL_RANK/WORLD_SIZE in the environment) each process
is one rank; launched plainly (`python bench.py --gpus N`) this process only SPAWNS the N ranks -- before anything here
touches a GPU -- relays rank 0's JSON line and exits with the worst return code.  The grid is partitioned in depth
(otmb_amd/dist.py):
    --scaling weak   (default) the global grid is the workload's horizontal grid with nz*N levels: per-GPU work fixed;
    --scaling strong the workload's own grid (e.g. --workload quarterdeg: BASELINE.json configs[3], the fixed
                     1440x1080x75 grid) cut into N depth slabs with balanced wet counts: total work fixed.
value = wet cells of all ranks / max-over-ranks time.  Prints ONE JSON line on rank 0.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy rate


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K timed steps are repeated R times; ms_per_step is the median (default: 1, with --full 5)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline too (see the module docstring); a plain run times the K steps and stops")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed as DIR/<name>.npy (float64, a fixed seeded sample; single GPU)")
    ap.add_argument("--workload", default="access1deg")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--rho", default="array", choices=["array", "scalar"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--end-to-end-large", action="store_true",
                    help="workloads generated on the device (quarterdeg): copy the grid down once and run the host-pointer end_to_end legs on it "
                         "(what a Julia caller waits for at BASELINE.json configs[2]; ~60 GB of host memory)")
    ap.add_argument("--given-ops", action="store_true",
                    help="profiling aid, never the driver's run: EVERY step of this process passes TκH and TκVdeep in (otmb_tm_args.given), so that a "
                         "rocprofv3 run of it averages the fill pass of that path alone (the default run measures it as the extra record given_ops_step)")
    ap.add_argument("--seed", type=int, default=20260501)
    ap.add_argument("--extra-configs", default="quarterdeg,tenthdeg",
                    help="after the headline workload (N = 1 only): BASELINE.json configs[2] (0.25 degree, the HBM-roofline run) and configs[4]'s "
                         "grid (0.1 degree, on ONE GPU) as extra records of the same JSON line; '' = none")
    ap.add_argument("--placement-candidates", type=int, default=4,
                    help="set-up, N = 1 only: DeviceAssembler.choose_placement -- the flux arrays and the output matrices are allocated this many times, "
                         "facefluxes / the fill pass timed on each, the fastest kept (profiles/r04/README.md section 12); 1 = off")
    ap.add_argument("--protocol", default="async", choices=["async", "twophase"],
                    help="async: otmb_transportmatrix_dev (count -> scan -> fill enqueued back to back, outputs preallocated "
                         "at their upper bound); twophase: plan (host learns nnz) then fill, as a caller that sizes its outputs does")
    args = ap.parse_args()
    if args.dump_outputs is not None and args.gpus != 1:
        ap.error("--dump-outputs needs --gpus 1")
    args.steps = max(1, args.steps)
    args.warmup = max(0, args.warmup)
    args.repeats = max(1, args.repeats if args.repeats is not None else (5 if args.full else 1))
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as child processes (this parent never
    initialises a GPU and never re-executes itself), relay rank 0's JSON line."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        # (the script that was started, not necessarily this file: tests/bench_rehearsal.py wraps main() and must be what the ranks run)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(sys.argv[0]), *sys.argv[1:]], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # poll every rank: when one dies the others would wait for it in a collective for ever -- stop them (they are this
    # process's own children) and report; an overall limit bounds the run whatever happens
    import threading

    out_chunks = []
    reader = threading.Thread(target=lambda: out_chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.time() + float(os.environ.get("OTMB_BENCH_TIMEOUT", "1500"))
    failed = None
    while any(p.poll() is None for p in procs):
        bad = [(r, p.returncode) for r, p in enumerate(procs) if p.poll() not in (None, 0)]
        if bad or time.time() > deadline:
            failed = bad[0] if bad else ("timeout", 124)
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            time.sleep(2)
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    rcs = [p.wait() for p in procs]
    if failed is None:  # (every rank ended between two polls, some of them badly: the first of those is named all the same)
        bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
        failed = bad[0] if bad else None
    reader.join(timeout=5)
    out = (out_chunks[0] if out_chunks else b"").decode()
    line = next((l for l in out.splitlines() if l.startswith("{")), None)
    if failed is not None:
        print(f"bench.py: rank {failed[0]} ended with status {failed[1]}; the other ranks were stopped", file=sys.stderr)
        return failed[1] if isinstance(failed[1], int) and failed[1] > 0 else 1
    if line:
        print(line, flush=True)
    return max(abs(rc) for rc in rcs) or (0 if line else 1)


class Watchdog:
    """A multi-rank run must END -- with a verdict -- whatever a collective does on first contact with a node: while armed, a phase that
    takes longer than its limit prints which rank was in which phase and ends THIS process with a non-zero status (os._exit: a thread
    stuck inside a collective cannot be unwound), which the launcher (torchrun, or bench.py's own spawn_ranks) turns into the end of
    the whole job.  OTMB_BENCH_PREFLIGHT_S (default 120) bounds the bring-up phases, OTMB_BENCH_WATCHDOG_S (default 1500) the rest."""

    def __init__(self, rank):
        import threading

        self.rank, self.lock, self.timer, self.threading = rank, threading.Lock(), None, threading
        self.absent = None  # callable -> the ranks that have not reported in yet (first_contact sets it once a store exists)

    def arm(self, phase, seconds):
        self.disarm()

        def expire():
            who = ""
            try:
                if self.absent is not None:
                    who = f"; ranks that never reached this phase: {self.absent()}"
            except Exception:
                pass
            print(f"bench.py: rank {self.rank} did not finish '{phase}' within {seconds:.0f} s{who} -- giving up (exit 3)", file=sys.stderr, flush=True)
            os._exit(3)

        with self.lock:
            self.timer = self.threading.Timer(seconds, expire)
            self.timer.daemon = True
            self.timer.start()

    def disarm(self):
        with self.lock:
            if self.timer is not None:
                self.timer.cancel()
                self.timer = None


def first_contact(dist, torch, world, rank, dev, backend, plane_elems, rehearsal, dog, full=True):
    """Evidence a multi-rank line must carry about ITS OWN communicator: how many ranks answered an all_reduce, which
    library / version carried it, and what the one exchange of the path costs here -- a (nx, ny) plane of ϕtop from rank r to rank r - 1
    (the facefluxes chain, src/velocities.jl:236-243 across depth slabs), whole and in the row bands it is handed over in.  Every phase
    runs under the watchdog.  Returns the record (every rank computes it; rank 0 prints it).  full=False (a plain run): the all_reduce
    alone, no hand-off timed."""
    limit = float(os.environ.get("OTMB_BENCH_PREFLIGHT_S", "120"))
    cdev = dev if backend == "nccl" else torch.device("cpu")
    rec = {"backend": backend, "world": world}
    # every rank signs in through the rendezvous store first, so that a watchdog that fires can NAME the ranks that never arrived
    if os.environ.get("OTMB_BENCH_TEST_STALL_RANK") == str(rank):  # fault injection (tests/test_bench_cpu.py): this rank never joins
        time.sleep(10 ** 6)
    try:
        store = dist.distributed_c10d._get_default_store()
        store.set(f"otmb_bench_signed_in_{rank}", "1")
        dog.absent = lambda: [r for r in range(world) if not store.check([f"otmb_bench_signed_in_{r}"])]
    except Exception:
        store = None
    dog.arm("preflight: all_reduce of ones", limit)
    ones = torch.ones(1, dtype=torch.float64, device=cdev)
    dist.all_reduce(ones)
    if cdev.type == "cuda":
        torch.cuda.synchronize(cdev)
    rec["ranks_seen"] = int(round(float(ones.item())))
    try:
        v = torch.cuda.nccl.version() if backend == "nccl" else None
        rec["library"] = ("RCCL " + ".".join(str(x) for x in v)) if v else ("gloo (torch %s)" % torch.__version__)
    except Exception as e:
        rec["library"] = f"unknown ({type(e).__name__})"
    rec["hip"] = getattr(torch.version, "hip", None)
    for k in ("NCCL_DEBUG", "NCCL_P2P_DISABLE", "NCCL_SOCKET_IFNAME", "RCCL_MSCCL_ENABLE", "HSA_ENABLE_IPC_MODE_LEGACY"):
        if k in os.environ:
            rec.setdefault("env", {})[k] = os.environ[k]
    # the chain's hand-off: rank r sends a plane to r - 1 (deepest slab first), timed between barriers; then the same in 4 row bands
    from otmb_amd import dist as odist

    comm = odist.Comm()
    pieces = int(os.environ.get("OTMB_CHAIN_PIECES", "0")) or (4 if plane_elems >= (1 << 19) else 1)
    if world > 1 and full:
        dog.arm("preflight: point-to-point plane hand-off", limit)
        send = torch.full((plane_elems,), float(rank), dtype=torch.float64, device=dev)
        recv = torch.empty(plane_elems, dtype=torch.float64, device=dev)

        def hand_off(nparts):
            step = (plane_elems + nparts - 1) // nparts
            hs, hr = [], []
            for q in range(nparts):
                a, b = q * step, min(plane_elems, (q + 1) * step)
                if rank + 1 < world:
                    hr.append(comm.irecv(recv[a:b], rank + 1))
                if rank > 0:
                    hs.append(comm.isend(send[a:b], rank - 1))
            for h in hr:
                comm.wait_recv(h)
            for h in hs:
                comm.wait_send(h)
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)

        out = {}
        for nparts in sorted({1, pieces}):
            hand_off(nparts)  # (first use of every pair's channel: connection set-up is not what a step pays)
            ts = []
            for _ in range(5):
                dist.barrier()
                t0 = time.perf_counter()
                hand_off(nparts)
                ts.append(time.perf_counter() - t0)
            t = torch.tensor([sorted(ts)[len(ts) // 2]], dtype=torch.float64, device=cdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            out[str(nparts)] = 1e3 * float(t.item())
        ok = bool(rank + 1 >= world or float(recv[0].item()) == float(rank + 1))
        okt = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=cdev)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        rec["plane_hand_off"] = {"bytes": 8 * plane_elems, "pieces": pieces, "ms_by_pieces": out, "payload_intact": bool(okt.item() == 1.0),
                                 "ms_per_piece": out[str(pieces)] / pieces,
                                 "what": "every rank r > 0 sends one (nx, ny) Float64 plane to rank r - 1 at once (non-blocking send / receive pairs, "
                                         "as dist.SlabRunner posts them), median of 5 between barriers, max over ranks"}
    dog.disarm()
    return rec


def cpu_baseline(g, gm, workload, reps=5):
    """The oracle (single-thread C restatement of the reference algorithm: push COO -> sparse() x4 ->
    3 sparse adds) timed on this box's host cores over the same workload: 1 warm-up + median of `reps`
    passes.  kind = "port": the Julia reference cannot run here (no julia binary; SURVEY.md
    section 8c)."""
    import numpy as np

    from oracle import oracle as orc

    orc.build()
    idx = orc.makeindices(gm.v3D)
    fill = g.umo.properties["_FillValue"]
    N = idx["N"]
    t_ff, t_tm = [], []
    for rep in range(reps + 1):
        t1 = time.perf_counter()
        phi = orc.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], fill, gm.gridtopology.kind)
        t2 = time.perf_counter()
        orc.transportmatrix(phi, gm, idx, g.rho, g.mlotst, g.kappaH, g.kappaVML, g.kappaVdeep, True, tight=True)
        t3 = time.perf_counter()
        if rep:  # the first pass is the warm-up
            t_ff.append(t2 - t1)
            t_tm.append(t3 - t2)
    ff, tm = float(np.median(t_ff)), float(np.median(t_tm))
    # second figure: the same algorithm on several host threads -- the four operator builds run
    # concurrently and the three adds are column-parallel (oracle/otmb_oracle.c, orc_transportmatrix_omp); the
    # scatter-then-sort formulation of the reference offers no more parallelism without being changed
    t_par = []
    for rep in range(4):
        t1 = time.perf_counter()
        orc.transportmatrix(phi, gm, idx, g.rho, g.mlotst, g.kappaH, g.kappaVML, g.kappaVdeep, True, tight=True, parallel=True)
        if rep:
            t_par.append(time.perf_counter() - t1)
    tmp = float(np.median(t_par))
    try:
        model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except (OSError, StopIteration):
        model = "unknown CPU"
    return {
        "value": N / (ff + tm), "unit": "wet-cells/s", "cores": 1, "kind": "port",
        "sample": f"facefluxes+transportmatrix on the full {workload} grid (N={N}), 1 warm-up + median of {reps} passes; "
                  f"facefluxes {ff:.3f} s, transportmatrix {tm:.3f} s (COO generation + sparse() x4 + 3 adds); "
                  f"host {os.cpu_count()} logical cores ({model}), 1 used",
        "seconds": ff + tm,
        "multithread": {"value": N / (ff + tmp), "unit": "wet-cells/s", "cores": min(orc.omp_threads(), os.cpu_count() or 1),
                        "seconds": ff + tmp,
                        "sample": f"same workload, OpenMP: 4 concurrent operator builds + column-parallel adds "
                                  f"({orc.omp_threads()} threads), transportmatrix {tmp:.3f} s, median of 3; facefluxes as above"},
    }


def kernel_source_hash():
    """profiles/traffic.json holds counter traffic measured for ONE version of the dominant kernel: it is keyed to a hash of
    the kernel's sources and ignored (traffic: null) when they have changed since."""
    h = hashlib.sha256()
    for f in ("otmb_transportmatrix.hip", "otmb_tm_column.h", "otmb_facefluxes.hip"):
        with open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def end_to_end(g, gm, asm_N, reps=5, warm=8, large=False):
    """What a Julia caller of the host-pointer C ABI sees (PCIe included; never `value`): facefluxesfrommasstransport +
    transportmatrix through otmb_amd.api on host arrays, median of `reps` time slices after `warm` warm-up slices (the first two slices of
    a loop allocate: device buffers, the pinned rings of the slab contexts, the pinned result blocks -- 123 and 31 ms against 23.4 ms from the
    third on, tools/onepass_loop.py; and the default call spends its first seven slices measuring which protocol this host is faster
    with, api.Trial).
    given_ops: the reference's own time-loop idiom (src/matrixbuilding.jl:133-147) -- TκH and TκVdeep, functions of the grid and κ alone, are
    built ONCE (buildTκH / buildTκVdeep) and passed back to every transportmatrix call, which then builds, and copies home, Tadv, TκVML and T only."""
    import numpy as np

    import otmb_amd
    import otmb_amd.api as api

    idx = api.makeindices(gm.v3D)
    res = {}
    # default: what `transportmatrix(; ϕ, ...)` does with no extension keyword -- on a grid of this size the pipelined one-phase build on 4
    # depth slabs of the GPU (api.default_slabs; otmb_mgpu_transportmatrix_onepass); two_phase: slabs=0, the plan -> allocate -> fetch call of
    # rounds 1-4; reuse: both reuse promises (then always two-phase: nothing is left to upload beside the download)
    t0 = time.perf_counter()
    H = api.buildTκH(gridmetrics=gm, indices=idx, ρ=g.rho, κH=g.kappaH)
    D = api.buildTκVdeep(mlotst=g.mlotst, gridmetrics=gm, indices=idx, κVdeep=g.kappaVdeep)
    build_ms = 1e3 * (time.perf_counter() - t0)
    given = {"TκH": H, "TκVdeep": D}
    legs = (("default", {}), ("two_phase", {"slabs": 0}), ("reuse", {"reuse_grid": True, "reuse_fluxes": True}),
            ("given", dict(given, reuse_grid=True)), ("given_no_promise", dict(given)), ("given_reuse", dict(given, reuse_grid=True, reuse_fluxes=True)))
    if large:  # (the 0.25 degree grid: a time slice moves 25 GB -- the legs that answer the questions asked of it, fewer repetitions)
        legs = (legs[0], legs[1], legs[3])
    pinned = {}
    for name, kw in legs:
        ts = []
        # (explicit protocols need two allocating slices, the measured default seven: api.Trial)
        for rep in range(reps + (warm if "slabs" not in kw else min(warm, 2))):
            t0 = time.perf_counter()
            phi = api.facefluxesfrommasstransport(umo=g.umo, vmo=g.vmo, gridmetrics=gm, indices=idx)
            t1 = time.perf_counter()
            tm = api.transportmatrix(ϕ=phi, mlotst=g.mlotst, gridmetrics=gm, indices=idx, ρ=g.rho, κH=g.kappaH, κVML=g.kappaVML,
                                     κVdeep=g.kappaVdeep, **kw)
            t2 = time.perf_counter()
            ts.append((t1 - t0, t2 - t1, api.last_call_seconds["plan"] + api.last_call_seconds["fetch"]))
            pinned[name] = {k: int(api.last_call_seconds[k]) for k in ("result_bytes_pinned", "result_bytes_used") if k in api.last_call_seconds}
            api.last_call_seconds.pop("result_bytes_pinned", None)
            api.last_call_seconds.pop("result_bytes_used", None)
            del tm, phi  # (a time-slice loop drops the previous matrices: their pinned blocks return to the context's pool)
        res[name] = tuple(float(np.median([x[q] for x in ts[-reps:]])) for q in range(3))
    if large:
        for name in ("reuse", "given_no_promise", "given_reuse"):
            res[name] = (float("nan"),) * 3
    ff, tm, cabi = res["default"]

    def protocol(**kw):
        tr = api.Trial.peek(0, int(asm_N), rho3d=np.ndim(g.rho) != 0, **kw)
        return "two-phase (rule)" if tr is None else ("pipelined" if tr.now else "two-phase") + " (measured by the first seven calls)"

    lib = __import__("otmb_amd.capi", fromlist=["lib"]).lib()
    given_rec = {
        "what": "transportmatrix(; ϕ, ..., TκH = H, TκVdeep = D, reuse_grid = true): the two grid-constant operators are built once "
                "(buildTκH / buildTκVdeep: build_operators_ms) and passed back every time slice, as src/matrixbuilding.jl:133-143 offers -- "
                "neither uploaded again, built, nor copied home; the very objects come back; T, Tadv, TκVML are the full call's bit for bit",
        "build_operators_ms": build_ms, "facefluxes_ms": 1e3 * res["given"][0], "transportmatrix_ms": 1e3 * res["given"][1],
        "transportmatrix_c_abi_ms": 1e3 * res["given"][2], "value": asm_N / (res["given"][0] + res["given"][1]),
        "protocol": protocol(reuse_grid=True, given=given),
        "transportmatrix_ms_no_promise": 1e3 * res["given_no_promise"][1], "value_no_promise": asm_N / (res["given_no_promise"][0] + res["given_no_promise"][1]),
        "no_promise": "the same call without reuse_grid: the two operators (and the grid) are uploaded and compared again every call",
        "transportmatrix_ms_reuse_fluxes": 1e3 * res["given_reuse"][1], "value_reuse_fluxes": asm_N / (res["given_reuse"][0] + res["given_reuse"][1]),
        "comparing_passes": int(lib.otmb_ctx_given_checks(api.context(0).handle)),
    }
    return {"value": asm_N / (ff + tm), "unit": "wet-cells/s", "facefluxes_ms": 1e3 * ff, "transportmatrix_ms": 1e3 * tm,
            "transportmatrix_c_abi_ms": 1e3 * cabi, "slabs": api.default_slabs(asm_N, int(g.umo.data.shape[2]), False, None),
            "default_protocol": protocol(), "given_ops": given_rec,
            "result_bytes": {"default": pinned.get("default"), "given": pinned.get("given"),
                             "note": "pinned host bytes of one result set of the pipelined call (capacities: the wet mask's bounds, the previous slice's "
                                     "counts + 25 / 50 % for Tadv / TκVML) against the bytes the matrices use; rounds 4-5 pinned 25 N entries for 19.2 N"},
            "transportmatrix_ms_two_phase": 1e3 * res["two_phase"][1], "value_two_phase": asm_N / (res["two_phase"][0] + res["two_phase"][1]),
            "facefluxes_ms_reuse": 1e3 * res["reuse"][0], "transportmatrix_ms_reuse": 1e3 * res["reuse"][1],
            "transportmatrix_c_abi_ms_reuse": 1e3 * res["reuse"][2], "value_reuse": asm_N / (res["reuse"][0] + res["reuse"][1]),
            "note": "host-pointer C ABI (what a Julia ccall passes): pageable host input arrays, five host CSC matrices out in pinned memory "
                    "of the library (otmb_host_alloc: the DMA writes them in place), PCIe both ways.  transportmatrix_ms: the default call -- "
                    "pipelined over `slabs` depth slabs of the GPU, a slab uploading while the one above it copies its columns home, row indices "
                    "and column offsets crossing the link as Int32 (otmb_mgpu_transportmatrix_onepass, OtmbXferItem.narrow); *_two_phase: slabs=0, otmb_transportmatrix_plan + _fetch (every upload before the "
                    "count, every download after it: rounds 1-4); c_abi_ms: inside the C calls; *_reuse: gridmetrics / indices uploaded once "
                    "(reuse_grid) and the face fluxes that facefluxes just computed not uploaded again (reuse_fluxes; two-phase)"}


def extra_configs_in_children(args):
    """The other single-GPU BASELINE configurations, each measured by a FRESH process of this same script (`--workload X`) that has the
    GPU to itself, BEFORE this process touches the GPU: where the allocator places an assembler's arrays moves the fill pass by +-10 %, and
    allocations made after another workload's blocks were freed measure up to 10 % slower than a fresh process's (profiles/r03/README.md,
    section 6) -- so every configuration is reported as what `python bench.py --workload X` prints.  Returns {key: record}."""
    names = {"quarterdeg": "config3", "tenthdeg": "config5"}
    out = {}
    for wl in [w for w in args.extra_configs.split(",") if w and w != args.workload]:
        key = names.get(wl, "config_" + wl)
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", wl, "--full", "--extra-configs", "", "--no-cpu-baseline", "--no-end-to-end",
               *(["--end-to-end-large"] if wl == "quarterdeg" and not args.no_end_to_end else []),
               "--steps", str(min(args.steps, 10)), "--warmup", "2", "--repeats", "2", "--rho", args.rho, "--seed", str(args.seed),
               "--placement-candidates", str(args.placement_candidates)]
        rec = {"workload": wl}
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=float(os.environ.get("OTMB_BENCH_EXTRA_TIMEOUT", "600")))
            line = next((l for l in r.stdout.decode().splitlines() if l.startswith("{")), None)
            if r.returncode != 0 or line is None:
                tail = r.stderr.decode()[-300:].replace("\n", " | ")
                rec["skipped" if "out of memory" in tail.lower() else "error"] = f"child exited with {r.returncode}: {tail}"
            else:
                d = json.loads(line)
                rec.update({"grid": d["config"]["workload"].split("grid ")[1].split(",")[0], "wet_cells": d["config"]["wet_cells"], "nnz": d["config"]["nnz"],
                            "protocol": d["config"]["protocol"], "steps": d["steps"], "warmup": d["warmup"], "ms_per_step": d["ms_per_step"],
                            "value": d["value"], "unit": d["unit"], "repeats": d["repeats"], "roofline": d["roofline"], "kernels_ms": d["kernels_ms"],
                            "step_gbs": d["step_gbs"], "placement": d.get("placement"), "fused_step": d.get("fused_step"), "given_ops_step": d.get("given_ops_step"),
                            "end_to_end": d.get("end_to_end"), "measured_by": "a fresh process: " + " ".join(cmd[1:6])})
        except subprocess.TimeoutExpired:
            rec["error"] = "child timed out"
        except Exception as e:  # an extra record must never cost the headline
            rec["error"] = f"{type(e).__name__}: {e}"[:300]
        out[key] = rec
    return out


def slab_config(workload, args, world, rank, dev, local_rank, rehearsal, backend, make_backend):
    """BASELINE.json configs[3] beside a multi-rank headline: the FIXED `workload` grid cut into `world` depth slabs (strong scaling),
    facefluxes chain planes over the communicator, asynchronous pipeline; K' = min(K, 10) steps x 2 repeats between barriers, max over
    ranks.  Every rank takes part; rank 0 returns the record."""
    import numpy as np
    import torch
    import torch.distributed as dist

    from otmb_amd import dist as odist
    from otmb_amd import synthetic, synthetic_device

    rec = {"workload": workload, "scaling": "strong", "n_gpus": world}
    nx, ny, nz, lf = synthetic.PRESETS[workload]
    counts = synthetic.level_wet_counts(nx, ny, nz, seed=args.seed, land_fraction=lf)
    k0, k1 = odist.balanced_partition(counts, world)[rank]
    dg = synthetic_device.make_device_grid((nx, ny, nz), dev, seed=args.seed, land_fraction=lf, rho=args.rho, k0=k0, k1=k1)
    local = odist.make_local_grid_from_device(dg)
    be = make_backend(local_rank)
    srun = odist.SlabRunner(be, odist.Comm(), local)

    def barrier():
        dist.barrier()
        if not rehearsal:
            torch.cuda.synchronize()

    k = min(args.steps, 10)
    for _ in range(2):
        srun.step_async(dg.umo, dg.vmo, dg.fill)
    srun.finish()
    be.sync()
    per = []
    for _ in range(2):
        barrier()
        t0 = time.perf_counter()
        for _ in range(k):
            srun.step_async(dg.umo, dg.vmo, dg.fill)
        srun.finish()
        be.sync()
        barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        per.append(float(t.item()) / k)
    ms = 1e3 * float(np.median(per))
    rec.update({"grid": f"{nx}x{ny}x{nz}", "rank0_levels": [int(k0), int(k1)], "wet_cells": int(srun.n_global),
                "nnz": dict(zip(("T", "Tadv", "TkH", "TkVML", "TkVdeep"), (int(x) for x in srun.nnz_global))), "protocol": "async",
                "steps": k, "ms_per_step": ms, "value": srun.n_global / (ms * 1e-3), "unit": "wet-cells/s",
                "ms_per_step_min": 1e3 * min(per), "ms_per_step_max": 1e3 * max(per)})
    del srun, be, dg, local
    import gc

    gc.collect()
    if not rehearsal:
        torch.cuda.empty_cache()
    return rec


def config2_bolus(g, gm, dev, local_rank, steps):
    """BASELINE.json configs[1] ("... incl. Redi/GM triads").  In the reference the triads never enter T (src/RediGM.jl:44; DESIGN.md
    section 0): the headline line IS config 2's transportmatrix (3-D ρ).  What the reference has of Redi/GM is bolus_GM_velocity
    (src/RediGM.jl:46-79): its two kernels on the same grid, device resident, as an extra record (never `value`).  Algorithmic bytes:
    ρ, Z3D (8 B), the wet byte and two (nx,ny) distances in, u and v out = 33 B per cell; the κGM·S intermediates are overhead."""
    import ctypes as C

    import numpy as np
    import torch

    from otmb_amd import capi

    ctx = capi.Context(local_rank)
    nx, ny, nz = gm.v3D.shape
    flat = lambda a: torch.from_numpy(np.asfortranarray(a, dtype=np.float64).ravel(order="F")).to(dev)
    dn = gm.distance_to_neighbour_2D
    rho, z3d, de, dnn = flat(g.rho), flat(gm.Z3D), flat(dn["east"]), flat(dn["north"])
    wet = (~torch.isnan(flat(gm.v3D))).to(torch.uint8)
    u, v = torch.empty_like(rho), torch.empty_like(rho)
    torch.cuda.synchronize(dev)

    def call():
        ctx.check(capi.lib().otmb_bolus_gm_velocity_dev(ctx.handle, rho.data_ptr(), z3d.data_ptr(), wet.data_ptr(), de.data_ptr(), dnn.data_ptr(),
                                                        nx, ny, nz, int(gm.gridtopology.kind), 600.0, 0.01, u.data_ptr(), v.data_ptr()))

    for _ in range(3):
        call()
    ctx.synchronize()
    ctx.timing_enable(True)
    for _ in range(steps):
        call()
    kt = ctx.timing_collect()
    ctx.timing_enable(False)
    ms = kt["gm_slopes+gm_dyad"][0] / kt["gm_slopes+gm_dyad"][1]
    G = nx * ny * nz
    alg = 33 * G + 16 * nx * ny
    ctx.close()
    return {"workload": f"bolus_GM_velocity on the {nx}x{ny}x{nz} grid (src/RediGM.jl:46-79; the reference's Redi/GM code never enters T)",
            "kernels": "gm_fused_kernel (κGM·S through LDS; OTMB_GM_FUSED=0: gm_slopes_kernel + gm_dyad_kernel)", "ms": ms, "cells_per_s": G / (ms * 1e-3), "algorithmic_bytes": alg,
            "achieved_gbs": alg / (ms * 1e-3) / 1e9, "frac_of_hbm_peak": alg / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "note": "4 arrays in (ρ, Z3D, wet, 2-D distances), 2 out; the two κGM·S arrays between the two steps stay in LDS.  Bound by its "
                    "arithmetic (~25 Float64 divisions and a tanh per cell in dependent chains), not by its bytes.  The transportmatrix of "
                    "config 2 (3-D ρ) is this line's headline."}


def box_probe(dev):
    """How fast is THIS box's memory system for the plainest job there is?  A 2 GiB device-to-device copy (torch), after the timed region: a
    reference point beside the line's own kernel times (the boxes of the pool differ by up to 15 % on the fill pass, profiles/r03/README.md
    section 6).  Not part of the measurement."""
    import torch
    n = 1 << 28
    a = torch.empty(n, dtype=torch.float64, device=dev).fill_(1.0)
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / reps
    return {"copy_2GiB_ms": ms, "copy_gbs_read_plus_write": 2 * n * 8 / (ms * 1e-3) / 1e9,
            "note": "torch device-to-device copy of 2 GiB after the timed region: this box's plain streaming rate.  (Round 3: the pool's boxes differ by up to 15 % on the "
                    "fill pass and this rate does not follow it -- 4.63 TB/s on a box with a 0.316 ms fill, 4.98 TB/s on one with 0.360 ms -- the pass is bound by "
                    "request latency, not by streaming bandwidth: profiles/r03/README.md 5b, 6.)"}


def rocm_smi_probe(index=0):
    """Clocks / power / temperature of the card, from a process that has NOT initialised the GPU (rocm-smi is an `env python3` script: started
    from a process whose GPU a HIP call or a profiler preload has initialised, every hop of that chain is an exec the GPU boxes refuse --
    profiles/r04 call 21, gpurun_out/.graft_exec_refused): only the launcher parent of bench.py calls this, right after the headline child."""
    try:
        r = subprocess.run(["rocm-smi", "-d", str(index), "--showclocks", "--showpower", "--showtemp", "--showmemuse", "--json"],
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=20)
        j = json.loads(r.stdout.decode() or "{}")
        card = next(iter(j.values())) if j else {}
        keep = ("sclk", "mclk", "fclk", "socclk", "Power", "Temperature", "junction", "memory", "GPU Memory Allocated")
        return {k: v for k, v in card.items() if any(t.lower() in k.lower() for t in keep)}
    except Exception as e:
        return {"error": f"{type(e).__name__}: {e}"[:120]}


def traffic_for(workload, kernel, args, world=1):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes (profiles/traffic.json), valid only for the
    kernel sources they were measured on (kernel_source_sha16) and for the workload they were measured at."""
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        if world != 1 or args.rho != "array" or tj.get("kernel_source_sha16") != kernel_source_hash():
            return None
        if getattr(args, "given_ops", False):  # the profiling run with TκH and TκVdeep passed in: its own PMC passes, its own kernel variant
            workload, kernel = workload + "_given", {"tm_kernel<fill>": "tm_kernel<fill, TκH read>"}.get(kernel, kernel)
        return tj.get("workloads", {}).get(workload, {}).get(kernel, {}).get("traffic_bytes")
    except (OSError, ValueError):
        return None


DUMP_SAMPLE = 1 << 16  # columns (and cells) sampled: <= 25 entries per column over the five matrices -> <= 32 MB in all


def dump_outputs(asm, outdir):
    """--dump-outputs: what the timed path handed back in its last step, for an output-by-output comparison of two builds on the same
    inputs.  Float64 .npy files in `outdir`: nnz.npy = [N, nnz of T, Tadv, TκH, TκVML, TκVdeep]; columns.npy = a sample of DUMP_SAMPLE
    column indices, fixed by a constant seed and N; per matrix <name>_colptr.npy (first and one-past-last entry of each sampled column),
    <name>_rowval.npy and <name>_nzval.npy (their entries, column after column); cells.npy and phi_<face>.npy: the six face fluxes on a
    sample of cells drawn the same way.  An operator passed in (--given-ops) was not written by the step and is left out."""
    import numpy as np
    import torch

    from otmb_amd.capi import MATS, PHI_ORDER

    asm.ctx.synchronize()
    os.makedirs(outdir, exist_ok=True)
    names = dict(zip(MATS, ("T", "Tadv", "TkH", "TkVML", "TkVdeep")))
    save = lambda name, a: np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    sample = lambda n: np.sort(np.random.default_rng(20260501).choice(n, size=min(n, DUMP_SAMPLE), replace=False))
    N = int(asm.N)
    save("nnz", [N, *asm.nnz])
    cols = sample(N)
    save("columns", cols)
    given = set(getattr(asm, "given", None) or ())
    for k, m in enumerate(MATS):
        if m in given:
            continue
        cp, rv, nz = asm.out[m]
        nnz = int(asm.nnz[k])
        if cp.numel() != N + 1 or rv.numel() < nnz or nz.numel() < nnz:
            raise RuntimeError(f"--dump-outputs: {m}'s buffers do not hold N + 1 offsets and {nnz} entries")
        base = int(cp[0].item())  # (1 for the reference's 1-based offsets)
        lo = cp[torch.from_numpy(cols).to(cp.device)].cpu().numpy() - base
        hi = cp[torch.from_numpy(cols + 1).to(cp.device)].cpu().numpy() - base
        if not (np.all(lo <= hi) and np.all(lo >= 0) and np.all(hi <= nnz)):  # checked here: an index beyond the arrays never reaches the device
            raise RuntimeError(f"--dump-outputs: {m}'s column offsets are not within [0, {nnz}]")
        cnt = hi - lo
        ent = np.repeat(lo - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt) + np.arange(int(cnt.sum()))
        ent_d = torch.from_numpy(ent).to(cp.device)
        save(names[m] + "_colptr", np.stack([lo, hi], axis=1))
        save(names[m] + "_rowval", rv[ent_d].cpu().numpy())
        save(names[m] + "_nzval", nz[ent_d].cpu().numpy())
    if getattr(asm, "phi", None) is not None:
        cells = sample(int(asm.G))
        save("cells", cells)
        cells_d = torch.from_numpy(cells).to(asm.phi[0].device)
        for face, p in zip(PHI_ORDER, asm.phi):
            save("phi_" + face, p[cells_d].cpu().numpy())


def under_profiler():
    """A rocprofv3 / rocprof preload has initialised the GPU before this script started: no child processes then (they would inherit the
    profiler, write their dispatches into the same output directory and mix two grids in one summary)."""
    return any(k.startswith(("ROCPROFILER_", "ROCPROF_")) for k in os.environ) or "rocprof" in os.environ.get("LD_PRELOAD", "")


def main(slab_backend_factory=None, cpu_rehearsal=False):
    """slab_backend_factory / cpu_rehearsal: a seam for tests/bench_rehearsal.py ONLY (the multi-rank plumbing of this script on a box
    without GPUs, over gloo, with a backend the TEST side supplies).  Nothing in this file imports from tests/ or oracle/ except the
    cpu_baseline leg, no environment variable or flag selects another backend: run as `python bench.py` the product library computes."""
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args))
    extras = {}
    if args.full and args.gpus == 1 and "RANK" not in os.environ and args.extra_configs and not cpu_rehearsal and not under_profiler():
        # Every configuration of the line is measured by a FRESH process that has the GPU to itself, the HEADLINE FIRST: a process that
        # starts after the 0.25 / 0.1 degree runs have allocated and freed 35 / 220 GB measures the same kernels 2-3 % slower
        # (profiles/r04/README.md section 7: 0.3775 against 0.3658 ms on one box; round 3 ran the headline last).  This process only
        # launches the others -- it never touches the GPU -- and prints the headline child's line with the extra records merged in.
        cmd = [sys.executable, os.path.abspath(sys.argv[0]), *[a for a in sys.argv[1:]], "--extra-configs", ""]
        head = None
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=float(os.environ.get("OTMB_BENCH_TIMEOUT", "1500")))
            line = next((l for l in r.stdout.decode().splitlines() if l.startswith("{")), None)
            if r.returncode == 0 and line is not None:
                head = json.loads(line)
        except (subprocess.TimeoutExpired, OSError, ValueError):
            head = None
        if head is not None:
            if isinstance(head.get("box_probe"), dict):
                head["box_probe"]["rocm_smi"] = rocm_smi_probe()  # this process never touches the GPU
            head.update(extra_configs_in_children(args))
            head["measured_by"] = "fresh processes, one per configuration, headline first: " + " ".join(cmd[1:])
            print(json.dumps(head), flush=True)
            return
        # (the headline child failed: measure it here, as rounds 1-3 did, so that the failure is visible in this process's output)
        extras = extra_configs_in_children(args)

    import numpy as np
    import torch
    import torch.distributed as dist

    import otmb_amd
    from otmb_amd import synthetic
    from otmb_amd.capi import MATS
    from otmb_amd.device import DeviceAssembler

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # OTMB_FORCE_SLAB=1: take the depth-slab (distributed) code path even with one rank, e.g. under
    # `torchrun --nproc-per-node 1`, to exercise RCCL initialisation and collectives on a one-GPU box
    force_slab = os.environ.get("OTMB_FORCE_SLAB") == "1" and "RANK" in os.environ
    if args.dump_outputs is not None and (force_slab or cpu_rehearsal):
        sys.exit("bench.py: --dump-outputs writes the single-GPU path's outputs; not with OTMB_FORCE_SLAB=1")
    # rehearsal (tests/bench_rehearsal.py only): the multi-rank orchestration of this script on a box without GPUs -- gloo, a
    # backend supplied by the test -- the line it prints is labelled as not being a measurement
    rehearsal = bool(cpu_rehearsal)
    saved_stdout_fd = None
    backend = os.environ.get("OTMB_DIST_BACKEND", "gloo" if rehearsal else "nccl")
    if world > 1 or force_slab:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # OTMB_DIST_BACKEND=gloo + OTMB_SHARE_GPU=1: rehearsal of the multi-rank path on a one-GPU box
        if os.environ.get("OTMB_SHARE_GPU") == "1":
            local_rank = 0
        if not rehearsal:
            # first contact: a node that shows fewer GPUs than ranks is the most likely first failure -- say so in one line, exit 3 like every
            # other bring-up failure (device_count() does not initialise the GPU)
            seen = torch.cuda.device_count()
            if local_rank >= seen:
                print(f"bench.py: rank {rank} (local rank {local_rank}): this node shows {seen} GPU(s) to this process, --gpus {world} needs "
                      f"{local_rank + 1} or more (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES: {os.environ.get('HIP_VISIBLE_DEVICES')!r} / "
                      f"{os.environ.get('ROCR_VISIBLE_DEVICES')!r})", file=sys.stderr)
                sys.exit(3)
            torch.cuda.set_device(local_rank)
        # RCCL prints a version banner on the process's stdout when its first communicator comes up; stdout must carry
        # exactly one JSON line, so file descriptor 1 points at stderr until the result is printed
        sys.stdout.flush()
        saved_stdout_fd = os.dup(1)
        os.dup2(2, 1)
        import datetime

        dog = Watchdog(rank)
        limit = float(os.environ.get("OTMB_BENCH_PREFLIGHT_S", "120"))
        dog.arm("init_process_group (" + backend + ")", limit + 30)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=datetime.timedelta(seconds=limit))
        else:
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=max(limit, 300)))
        dog.disarm()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    dev = torch.device("cpu") if rehearsal else torch.device("cuda", local_rank)
    comm_rec = None
    if world > 1 or force_slab:
        nx_, ny_ = synthetic.PRESETS[args.workload][:2]
        comm_rec = first_contact(dist, torch, world, rank, dev, backend, nx_ * ny_, rehearsal, dog, full=args.full)
        if comm_rec["ranks_seen"] != world:
            print(f"bench.py: rank {rank}: all_reduce saw {comm_rec['ranks_seen']} of {world} ranks", file=sys.stderr, flush=True)
            os._exit(4)
        dog.arm("the measurement", float(os.environ.get("OTMB_BENCH_WATCHDOG_S", "1500")))

    def make_backend(lr):
        if slab_backend_factory is not None:
            assert rehearsal, "a foreign slab backend is a rehearsal, never a measurement"
            return slab_backend_factory(lr)
        from otmb_amd import dist as odist_

        return odist_.HipSlabBackend(lr)

    # One arena for everything the run allocates: a block of the workload's whole footprint is reserved and handed back to
    # torch's caching allocator BEFORE anything else is allocated, so that every array of the run is carved out of one device
    # allocation (one contiguous range of addresses) instead of one hipMalloc per array (placement: profiles/r04/README.md section 7).
    arena_gb = float(os.environ.get("OTMB_BENCH_ARENA_GB", "0"))
    if arena_gb > 0 and not rehearsal:
        _arena = torch.empty(int(arena_gb * 2 ** 30), dtype=torch.uint8, device=dev)
        del _arena

    nx, ny, nz, lf = synthetic.PRESETS[args.workload]
    host_grid = None  # (g, gm) when the whole grid also exists on the host (cpu_baseline / end_to_end legs)
    placement = None  # DeviceAssembler.choose_placement's record (single-GPU, asynchronous protocol)
    if world > 1 or force_slab:
        from otmb_amd import dist as odist
        from otmb_amd import synthetic_device

        # weak: nz*world levels stretched over the same depth, per-GPU work fixed; strong: the workload's own grid
        nzg = nz * world if args.scaling == "weak" else nz
        counts = synthetic.level_wet_counts(nx, ny, nzg, seed=args.seed, land_fraction=lf)
        k0, k1 = odist.balanced_partition(counts, world)[rank]
        # every rank generates only its own levels, on its own device
        dg = synthetic_device.make_device_grid((nx, ny, nzg), dev, seed=args.seed, land_fraction=lf, rho=args.rho, k0=k0, k1=k1)
        local = odist.make_local_grid_from_device(dg)
        be = make_backend(local_rank)
        srun = odist.SlabRunner(be, odist.Comm(), local)
        umo, vmo, fill = dg.umo, dg.vmo, dg.fill

        class _Slab:
            n_wet_total = srun.n_global
            ctx = getattr(be, "ctx", None)
            pending = False
            slab = (k0, k1, nzg)

            def step(self):
                # always the asynchronous pipeline: only the facefluxes chain's planes couple the ranks (the synchronous
                # SlabRunner.step gathers nnz with two collectives per field: every rank would wait out the chain's skew every step)
                srun.step_async(umo, vmo, fill)
                self.pending = True

            def sync(self):
                if self.pending:
                    srun.finish()
                    self.pending = False
                be.sync()

            @property
            def nnz(self):
                return [int(x) for x in srun.nnz_global]

            def algorithmic_bytes(self):  # this rank's slab (rank 0 reports)
                n3d = 9 + (1 if be.rho is not None else 0)
                return 8 * be.G * n3d + 80 * nx * ny + 8 * be.nz + sum(16 * z + 8 * (be.n_own + 1) for z in be.nnz)

            def facefluxes_bytes(self):
                return be.nown_lev * be.P * (16 + 1 + 48)

        runner = _Slab()
    else:
        if args.workload in ("quarterdeg", "tenthdeg"):  # too large to build on the host and copy: generated on the device
            from otmb_amd import synthetic_device

            dg = synthetic_device.make_device_grid(args.workload, dev, seed=args.seed, rho=args.rho)
            asm = synthetic_device.assembler_for(dg, local_rank)
            umo, vmo, fill = dg.umo, dg.vmo, dg.fill
        else:
            g = synthetic.make_grid(nx, ny, nz, seed=args.seed, land_fraction=lf, rho=args.rho)
            gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                          lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
            host_grid = (g, gm)
            asm = DeviceAssembler(local_rank)
            asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=True)
            umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).to(dev)
            vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).to(dev)
            fill = g.umo.properties["_FillValue"]

        # (not under a profiler: the candidates' launches would enter the per-kernel averages of profiles/*_kernel_stats.csv and traffic.json)
        if args.placement_candidates > 1 and args.protocol == "async" and args.workload != "tenthdeg" and not under_profiler():
            try:  # set-up, outside the timed region; never results (tests/test_device_api.py)
                placement = asm.choose_placement(umo, vmo, fill, candidates=args.placement_candidates)
            except Exception as e:
                placement = {"error": f"{type(e).__name__}: {e}"[:200]}

        class _Single:
            protocol = "twophase" if (args.protocol == "twophase" or args.workload == "tenthdeg") else "async"
            n_wet_total = asm.N
            ctx = asm.ctx
            pending = False
            slab = (0, nz, nz)

            def step(self):
                if args.protocol == "async" and args.workload != "tenthdeg":
                    asm.step_async(umo, vmo, fill)  # no host round trip inside a step; errors surface in sync()
                    self.pending = True
                else:  # (the upper-bound output buffers of the asynchronous protocol do not fit at 0.1 degree)
                    asm.step(umo, vmo, fill, onepass=False)

            def sync(self):
                if self.pending:
                    asm.finish()
                    self.pending = False
                asm.ctx.synchronize()

            @property
            def nnz(self):
                return asm.nnz

            def algorithmic_bytes(self):
                return asm.algorithmic_bytes()

            def facefluxes_bytes(self):
                return asm.facefluxes_bytes()

            def bytes_split(self, fill_pass):  # (read, written) of the dominant kernel
                return asm.algorithmic_bytes_split() if fill_pass else (asm.G * 17, asm.G * 48)

            def stream_mix(self):
                return asm.fill_pass_stream_mix()

            def fused_step(self):  # the extension otmb_step_dev: only ϕtop stored (never `value`: the two-call path is the drop-in)
                asm.step_fused_async(umo, vmo, fill)

            fused_available = args.protocol == "async" and args.workload != "tenthdeg" and nx >= 3
            given_available = args.protocol == "async" and args.workload != "tenthdeg" and not args.given_ops and not under_profiler()

            def given_steps(self, args, barrier):
                full_nnz = list(asm.nnz)
                full_r, full_w = asm.algorithmic_bytes_split()
                ops = {}
                for m in ("TκH", "TκVdeep"):  # this grid's own operators, as a caller keeps them: exact-length copies of the last step's
                    k = asm.nnz[MATS.index(m)]
                    cp, rv, nz = asm.out[m]
                    ops[m] = (cp.clone(), rv[:k].clone(), nz[:k].clone())
                asm.set_given(**ops)
                try:
                    for _ in range(max(args.warmup, 2)):
                        asm.step_async(umo, vmo, fill)
                    asm.finish()
                    states = [asm.ctx.given_state(MATS.index(m)) for m in ("TκH", "TκVdeep")]
                    reps = []
                    for _ in range(min(args.repeats, 3)):
                        barrier()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            asm.step_async(umo, vmo, fill)
                        asm.finish()
                        barrier()
                        reps.append(time.perf_counter() - t0)
                    asm.ctx.timing_enable(True)
                    for _ in range(args.steps):
                        asm.step_async(umo, vmo, fill)
                    asm.finish()
                    gk = asm.ctx.timing_collect()
                    asm.ctx.timing_enable(False)
                    r, w = asm.algorithmic_bytes_split()
                    gms = 1e3 * float(np.median(reps)) / args.steps
                    fill_ms = gk["tm_kernel<fill>"][0] / gk["tm_kernel<fill>"][1]
                    same = asm.nnz[0] == full_nnz[0] and asm.nnz[1] == full_nnz[1] and asm.nnz[3] == full_nnz[3]
                    checks = int(asm.lib.otmb_ctx_given_checks(asm.ctx.handle))
                    # ... and the same two operators as a caller holds them who built them with ANOTHER κ (the call's own κH / κVdeep left at their
                    # defaults): the derived rows, other values -- the fill pass reads both where they lie (tm_kernel<., 3>)
                    other = None
                    try:
                        ops["TκH"][2].mul_(0.5); ops["TκVdeep"][2].mul_(3.0)  # (in place: the assembler tells the library to look again)
                        for _ in range(2):
                            asm.step_async(umo, vmo, fill)
                        asm.finish()
                        ostates = [asm.ctx.given_state(MATS.index(m)) for m in ("TκH", "TκVdeep")]
                        barrier()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            asm.step_async(umo, vmo, fill)
                        asm.finish()
                        barrier()
                        oms = 1e3 * (time.perf_counter() - t0) / args.steps
                        asm.ctx.timing_enable(True)
                        for _ in range(args.steps):
                            asm.step_async(umo, vmo, fill)
                        asm.finish()
                        ok_ = asm.ctx.timing_collect()
                        asm.ctx.timing_enable(False)
                        other = {"what": "the two operators built with another κ (derived rows, other values): read by the fill pass, no sparse add, every protocol",
                                 "given_state": ostates, "ms_per_step": oms, "kernels_ms": {k: round(v[0] / v[1], 5) for k, v in ok_.items()}}
                    except Exception as e:  # an extra record must never cost the line
                        other = {"error": f"{type(e).__name__}: {e}"[:200]}
                    return {"what": "transportmatrix with TκH and TκVdeep GIVEN (otmb_tm_args.given; src/matrixbuilding.jl:133-147), device resident, two-call "
                                    "path; an extra record, NOT the headline: the two operators are neither counted nor written -- the fill pass reads TκH's "
                                    "values where they lie and re-derives TκVdeep's in registers (verdict of ONE comparing pass, cached); T is the same bit for bit",
                            "other_kappa": other,
                            "given_state": dict(zip(("TκH", "TκVdeep"), ("derived" if q == 1 else "foreign" if q == 2 else "derived rows, other values" if q == 3 else "not given" for q in states))),
                            "ms_per_step": gms, "wet_cells_per_s": asm.N / (gms * 1e-3), "kernels_ms": {k: round(v[0] / v[1], 5) for k, v in gk.items()},
                            "fill_bytes": {"read": r, "written": w, "total": r + w, "full_build_total": full_r + full_w},
                            "fill_gbs": (r + w) / (fill_ms * 1e-3) / 1e9, "fill_frac_of_hbm_peak": (r + w) / (fill_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                            "nnz_T_Tadv_TkVML_as_in_the_full_build": bool(same), "comparing_passes": checks}
                finally:
                    asm.set_given(TκH=None, TκVdeep=None)
                    asm.step_async(umo, vmo, fill)  # (the full build again: the roofline record below reads this object's nnz and matrices)
                    asm.finish()

        runner = _Single()
        if args.given_ops:  # (profiling aid: see the flag) this grid's own two grid-constant operators, passed back to every step from here on
            asm.step(umo, vmo, fill)
            ops = {}
            for m in ("TκH", "TκVdeep"):
                k = asm.nnz[MATS.index(m)]
                cp, rv, nz_ = asm.out[m]
                ops[m] = (cp.clone(), rv[:k].clone(), nz_[:k].clone())
            asm.set_given(**ops)

    def barrier():
        if dist.is_initialized():
            dist.barrier()
        if not rehearsal:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        runner.step()
    runner.sync()
    # EXACTLY K steps between two barrier + synchronize brackets, max over ranks; repeated R times: the pool's boxes
    # differ by ~15 % and a single 10 ms region says little, so the median is reported with the spread beside it
    per_repeat = []
    for _ in range(args.repeats):
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            runner.step()
        runner.sync()
        barrier()
        elapsed = time.perf_counter() - t0
        if dist.is_initialized():
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        per_repeat.append(elapsed)
    elapsed = float(np.median(per_repeat))
    if args.dump_outputs is not None:  # (before anything below runs other steps or overwrites the matrices)
        dump_outputs(asm, args.dump_outputs)

    # per-kernel durations with HIP events on the launch stream, over one more pass of the same K steps
    ktimes = {}
    if runner.ctx is not None and args.full:
        runner.ctx.timing_enable(True)
        for _ in range(args.steps):
            runner.step()
        runner.sync()
        ktimes = runner.ctx.timing_collect()
        runner.ctx.timing_enable(False)

    # The fused device-resident step (otmb_step_dev: facefluxes stores ϕtop only, the fill pass re-derives the other five fluxes from umo /
    # vmo; the same five matrices bit for bit, tests/test_fused_step.py), measured the same way right after the headline and reported as an
    # EXTRA record: `value` stays the two-call path, which is what the reference's API is (facefluxesfrommasstransport returns six arrays).
    fused = None
    if getattr(runner, "fused_available", False) and not rehearsal and args.full:
        try:
            for _ in range(args.warmup):
                runner.fused_step()
            runner.pending = True
            runner.sync()
            reps = []
            for _ in range(min(args.repeats, 3)):
                barrier()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    runner.fused_step()
                runner.pending = True
                runner.sync()
                barrier()
                reps.append(time.perf_counter() - t0)
            runner.ctx.timing_enable(True)
            for _ in range(args.steps):
                runner.fused_step()
            runner.pending = True
            runner.sync()
            fk = runner.ctx.timing_collect()
            runner.ctx.timing_enable(False)
            fms = 1e3 * float(np.median(reps)) / args.steps
            fused = {"what": "otmb_step_dev (extension, NOT the headline): one call from (umo, vmo) to the five matrices, only ϕtop stored -- "
                             "64 bytes per cell less HBM traffic; the same matrices bit for bit",
                     "ms_per_step": fms, "wet_cells_per_s": runner.n_wet_total / (fms * 1e-3),
                     "kernels_ms": {k: round(v[0] / v[1], 5) for k, v in fk.items()}}
        except Exception as e:  # an extra record must never cost the headline
            fused = {"error": f"{type(e).__name__}: {e}"[:300]}

    # The reference's time-loop shortcut on the device (otmb_tm_args.given): TκH and TκVdeep of this grid passed back to every step -- derived
    # (one comparing pass, then cached), so the fill pass neither counts nor writes them.  An EXTRA record (never `value`: the headline returns
    # all five matrices); measured like the headline, two-call path (facefluxes -> transportmatrix).
    given_step = None
    if getattr(runner, "given_available", False) and not rehearsal and args.full:
        try:
            given_step = runner.given_steps(args, barrier)
        except Exception as e:  # an extra record must never cost the headline
            given_step = {"error": f"{type(e).__name__}: {e}"[:300]}

    # N > 1: BASELINE.json configs[3] (the fixed 0.25 degree grid cut into N depth slabs) beside the headline, unless it IS the headline
    config4 = None
    c4_workload = os.environ.get("OTMB_BENCH_CONFIG4_WORKLOAD", "quarterdeg")  # (tests rehearse this leg on a small grid)
    if world > 1 and args.full and args.extra_configs and not (args.workload == c4_workload and args.scaling == "strong") and \
            (not rehearsal or "OTMB_BENCH_CONFIG4_WORKLOAD" in os.environ):
        try:
            config4 = slab_config(c4_workload, args, world, rank, dev, local_rank, rehearsal, backend, make_backend)
        except Exception as e:  # every rank raises the same pipeline errors (dist.SlabRunner.finish), so nobody is left in a collective
            config4 = {"workload": c4_workload, "error": f"{type(e).__name__}: {e}"[:300]}
    kernels_by_rank = None
    if dist.is_initialized() and (world > 1 or force_slab) and args.full:
        mine = {k: v[0] / v[1] for k, v in ktimes.items()}
        allk = [None] * world
        dist.all_gather_object(allk, mine)
        names = sorted({k for d_ in allk for k in d_})
        kernels_by_rank = {k: {"min": round(min(d_.get(k, float("inf")) for d_ in allk), 5), "max": round(max(d_.get(k, 0.0) for d_ in allk), 5)}
                           for k in names}
    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        n_total = runner.n_wet_total
        value = n_total * args.steps / elapsed
        kavg = {k: v[0] / v[1] for k, v in ktimes.items()}
        roof = None
        if kavg:
            dom = max(kavg, key=kavg.get)
            bytes_alg = runner.algorithmic_bytes() if dom.startswith(("tm_kernel", "dm_fill")) else runner.facefluxes_bytes()
            achieved = bytes_alg / (kavg[dom] * 1e-3) / 1e9
            traffic = traffic_for(args.workload, dom, args, world)
            roof = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "algorithmic_bytes_per_launch": bytes_alg,
                    "avg_kernel_ms": kavg[dom]}
        if roof is not None and world == 1 and not force_slab and not rehearsal and hasattr(runner, "bytes_split"):
            # The same kernel time as a fraction of what THIS box sustains: one plain read stream and one plain non-temporal write stream
            # (otmb_ctx_box_ceilings, measured here, in this process, right after the timed region), combined for the kernel's own read : write
            # mix -- bytes / (reads / read rate + writes / write rate).  The pool's boxes differ by up to 15 % on the same binary.
            try:
                rd, wr = runner.ctx.box_ceilings()
                br, bw = runner.bytes_split(dom.startswith(("tm_kernel", "dm_fill")))
                mix = (br + bw) / (br / rd + bw / wr)
                roof["box"] = {"read_gbs": rd, "write_gbs": wr, "mix_ceiling": mix, "frac_of_box": achieved / mix,
                               "bytes_read": br, "bytes_written": bw}
                if dom.startswith("tm_kernel") and hasattr(runner, "stream_mix") and not args.given_ops:
                    # ... and of what an ideal streaming kernel reaches over the fill pass's OWN arrays, where they lie (destroys the matrices:
                    # everything that reads them has run).  The two plain streams above are the same on fast and slow boxes (profiles/r05).
                    sm = runner.stream_mix()  # {columns per slice: GB/s}; 256 = the fill pass's own tile
                    roof["box"]["stream_mix_gbs"] = {str(k): v for k, v in sm.items()}
                    roof["box"]["frac_of_mix"] = achieved / max(sm.values())  # against the BEST plain stream over these arrays
            except Exception as e:  # a diagnostic must never cost the line
                roof["box"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        k0, k1, nzg = runner.slab
        if world > 1:
            shape = (f"{nx}x{ny}x{nzg} cut into {world} depth slabs (rank 0: levels [{k0},{k1}))"
                     + (f"; weak scaling: {nz} levels per rank" if args.scaling == "weak" else "; strong scaling: fixed grid"))
        else:
            shape = f"{nx}x{ny}x{nz}"
        out = {
            "metric": "wet-cells/s assembled into T" if not rehearsal else "REHEARSAL of the multi-rank orchestration (CPU checker backend): not a measurement",
            "value": value, "unit": "wet-cells/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": args.scaling if world > 1 else "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic", "full": bool(args.full),
            "config": {
                "workload": f"{args.workload}: synthetic ACCESS-ESM1-5-like tripolar grid {shape}"
                            f", facefluxes + full transportmatrix (5 CSC matrices), rho={args.rho}, upwind"
                            + (" -- PROFILING RUN with TκH and TκVdeep passed in (--given-ops): 3 matrices built, not the headline" if args.given_ops else ""),
                "wet_cells": n_total, "nnz": dict(zip(("T", "Tadv", "TkH", "TkVML", "TkVdeep"), runner.nnz)),
                "seed": args.seed, "protocol": getattr(runner, "protocol", args.protocol),
            },
            "repeats": {"n": args.repeats, "ms_per_step_median": ms_step, "ms_per_step_min": 1e3 * min(per_repeat) / args.steps,
                        "ms_per_step_max": 1e3 * max(per_repeat) / args.steps},
            "roofline": roof,
            "kernels_ms": {k: round(v, 5) for k, v in kavg.items()},
            "step_gbs": None if rehearsal else (runner.algorithmic_bytes() + runner.facefluxes_bytes()) / (ms_step * 1e-3) / 1e9,
        }
        if fused is not None:
            out["fused_step"] = fused
        if given_step is not None:
            out["given_ops_step"] = given_step
        if world == 1 and not force_slab and not rehearsal:
            out["placement"] = placement
        if world > 1 or force_slab:
            out["config"]["ranks_over"] = backend  # the depth-slab path: "nccl" = RCCL (one rank per GPU)
            out["config"]["ranks_seen"] = comm_rec["ranks_seen"]  # an all_reduce of ones over the group, before anything was measured
            out["comm"] = comm_rec
            out["kernels_ms_over_ranks"] = kernels_by_rank
            if world > 1 and kernels_by_rank and comm_rec.get("plane_hand_off"):
                # what a weak-scaled step should cost: the slowest rank's own kernels + one hand-off per chain piece
                own = sum(v["max"] for k, v in kernels_by_rank.items() if k in ("facefluxes_kernel", "tilescan_kernel", "tm_kernel<fill>", "tm_count_kernel"))
                out["comm"]["expected_step_ms"] = own + comm_rec["plane_hand_off"]["ms_by_pieces"][str(comm_rec["plane_hand_off"]["pieces"])]
                out["comm"]["expected_step_note"] = "slowest rank's facefluxes + scan + fill (HIP events) + one plane hand-off; the measured ms_per_step above it is orchestration and skew"
        if world == 1 and host_grid is not None and not rehearsal and args.full:
            try:  # (an extra record must never cost the headline: the host-pointer legs allocate gigabytes of pinned memory and start threads)
                out["end_to_end"] = None if args.no_end_to_end else end_to_end(*host_grid, n_total)
            except Exception as e:
                out["end_to_end"] = {"error": f"{type(e).__name__}: {e}"[:300]}
            out["cpu_baseline"] = None if args.no_cpu_baseline else cpu_baseline(*host_grid, args.workload)
        if world == 1 and host_grid is None and args.end_to_end_large and not rehearsal and not force_slab and args.full:
            try:  # (after everything that reads the assembler's matrices: it is released first -- the host-pointer engines stage the grid themselves)
                import gc

                from otmb_amd import synthetic_device as _sd

                hg = _sd.host_copy(dg)
                del asm, runner
                gc.collect()
                torch.cuda.empty_cache()
                out["end_to_end"] = end_to_end(*hg, n_total, reps=3, warm=8, large=True)
            except Exception as e:
                out["end_to_end"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        if world == 1 and host_grid is not None and not rehearsal and dev.type == "cuda" and args.full:
            try:  # an extra record must never cost the headline
                out["config2"] = config2_bolus(*host_grid, dev, local_rank, min(args.steps, 10))
            except Exception as e:
                out["config2"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        if world == 1 and not rehearsal and dev.type == "cuda" and args.full:
            try:  # after the timed region and not part of the measurement: it must never cost the line
                torch.cuda.empty_cache()
                out["box_probe"] = box_probe(dev)
            except Exception as e:
                out["box_probe"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        if config4 is not None:
            out["config4"] = config4
        out.update(extras)  # BASELINE.json configs[2] ("HBM-roofline run") and the grid of configs[4] on this one GPU
        sys.stdout.flush()
        if saved_stdout_fd is not None:
            os.dup2(saved_stdout_fd, 1)
        print(json.dumps(out), flush=True)
        if saved_stdout_fd is not None:
            os.dup2(2, 1)  # anything the communicator says while shutting down goes to stderr too
    if dist.is_initialized():
        if world > 1 or force_slab:
            dog.arm("the closing barrier", 120.0)
        dist.barrier()
        dist.destroy_process_group()
        if world > 1 or force_slab:
            dog.disarm()


if __name__ == "__main__":
    main()
