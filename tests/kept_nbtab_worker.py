"""Scenarios of tests/test_kept_nbtab.py, importable and runnable as a child process: the neighbour-table switch (OTMB_KEPT_NBTAB) is read once
per process, so the OTMB_KEPT_NBTAB=0 (today's gathers) side of every comparison runs here and writes its digests to a JSON file.

    python tests/kept_nbtab_worker.py OUT.json        (needs a GPU)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers  # noqa: E402
from helpers import COUNTS_ON  # noqa: E402
from kept_htab_worker import digest, launches  # noqa: E402

# the grids of the comparison beyond helpers.CASES: the smallest at which each thing can go wrong
# (name: make_grid's arguments, randomize the metrics? -- as helpers.CASES does where the geometry is degenerate: at nx = 3 the geometric
# distances make the reference itself fail with "TκH contains NaNs")
EXTRA = {
    "nb_3x3x1": (dict(nx=3, ny=3, nz=1, land_fraction=0.0), True),   # the narrowest fast path: no A / B, E and W are each other's wrap
    "nb_3x4x2": (dict(nx=3, ny=4, nz=2, land_fraction=0.0), True),   # ... with one vertical neighbour
    "nb_10x8x1": (dict(nx=10, ny=8, nz=1), False),                    # no vertical neighbours, some land
    "nb_20x12x5_land60": (dict(nx=20, ny=12, nz=5, land_fraction=0.6), False),  # most neighbours absent
}


def pair(name, upwind=True):
    """test_kept_ops._pair, also for the grids of EXTRA (built here: helpers.CASES is other tests' list too and stays as it is)."""
    from test_kept_ops import _pair

    if name not in EXTRA:
        return _pair(name, upwind=upwind)
    import torch

    from otmb_amd import synthetic
    from otmb_amd.device import DeviceAssembler

    kw = dict(EXTRA[name][0])
    g = synthetic.make_grid(kw.pop("nx"), kw.pop("ny"), kw.pop("nz"), **kw)
    gm = helpers.gridmetrics_of(g)
    if EXTRA[name][1]:
        helpers.randomize_metrics(gm)
    asms = []
    for _ in range(2):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=upwind)
        asms.append(a)
    asms[1]._kept_ops = lambda out: (0, ())
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    return g, gm, asms[0], asms[1], umo, vmo, g.umo.properties["_FillValue"]


NAMES = ["tiny_tripolar", "tiny_bipolar", "odd_nx_fold", "even_fold_open", "float32_flux", "small_rho3d", *EXTRA]
PROTOCOLS = ["async", "pipeline", "fused", "twophase"]
KEPT = ("TκH", "TκVML", "TκVdeep")


def cases():
    return [(n, u, p) for n in NAMES for u in (True, False) for p in PROTOCOLS if p != "fused" or COUNTS_ON]


def run_case(name, upwind, protocol, steps=5, with_full=True):
    """The kept assembler (and one that never promises) over `steps` changing flux fields: per step the digests, and which steps kept."""
    from test_kept_ops import _fields, _run

    g, gm, asm, full, umo, vmo, fill = pair(name, upwind=upwind)
    asm.ctx.timing_enable(True)
    rec = {"kept": [], "full": [], "kept_steps": []}
    for u, v in _fields(umo, vmo, steps, seed=len(name)):
        _run(asm, protocol, u, v, fill)
        rec["kept"].append(digest(asm))
        if with_full:
            _run(full, protocol, u, v, fill)
            rec["full"].append(digest(full))
        rec["kept_steps"].append(asm._kept_last == KEPT)
    rec["launches"] = launches(asm)
    rec["kept_nbtab"] = asm.ctx.kept_nbtab()
    asm.ctx.timing_enable(False)
    return rec


def two_wet_cells(asm):
    """Linear indices of the first two wet cells."""
    L = asm.lwet[:2].cpu().numpy() - 1
    return int(L[0]), int(L[1])


def run_noncanonical_pipeline(steps=4):
    """Lwet3D with the ranks of two wet cells swapped, then a `steps`-step asynchronous pipeline: (error text, failing step), every step's status."""
    from otmb_amd.capi import OtmbError
    from test_kept_ops import _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    a, b = two_wet_cells(asm)
    ra, rb = int(asm.lwet3d[a]), int(asm.lwet3d[b])
    asm.lwet3d[a], asm.lwet3d[b] = rb, ra
    err = None
    try:
        for _ in range(steps):
            asm.step_async(umo, vmo, fill)
        asm.finish()
    except OtmbError as e:
        err = (str(e), e.step)
    return {"error": err, "steps": [list(asm.result_step(k)) for k in range(steps)]}


def main(path):
    res = {"cases": {f"{n}|{u}|{p}": run_case(n, u, p, with_full=False) for n, u, p in cases()}, "noncanonical": run_noncanonical_pipeline()}
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
