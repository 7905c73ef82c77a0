"""Scenarios of tests/test_kept_vrtab.py, importable and runnable as a child process: the {v3D, ρ} table switch (OTMB_KEPT_VRTAB) is read once
per process, so the OTMB_KEPT_VRTAB=0 (today's gathers) side of every comparison runs here and writes its digests to a JSON file.

    python tests/kept_vrtab_worker.py OUT.json        (needs a GPU)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers  # noqa: E402
from helpers import COUNTS_ON  # noqa: E402
from kept_htab_worker import digest, launches, wet_regular_cell  # noqa: E402

# the grids of the comparison beyond helpers.CASES, all with a 3-D ρ (name: make_grid's arguments)
EXTRA = {
    "vr_20x12x5_land60": dict(nx=20, ny=12, nz=5, land_fraction=0.6, rho="array"),  # most neighbours absent: they load the column's own record
    "vr_20x12x1_island": dict(nx=20, ny=12, nz=1, land_fraction=0.6, seed=16, rho="array"),  # one wet cell with no wet neighbour at all
}
# wet columns: 440, 6962, 430, 102 -- none a multiple of 64 or 256; small_rho3d spans 28 tiles of 256 columns
NAMES = ["tiny_rho3d", "small_rho3d", *EXTRA]
PROTOCOLS = ["async", "pipeline", "fused", "twophase"]
KEPT = ("TκH", "TκVML", "TκVdeep")


def grid(name):
    """(g, gm) of a case of helpers.CASES or of EXTRA."""
    from otmb_amd import synthetic

    if name not in EXTRA:
        return helpers.make_case(name)
    kw = dict(EXTRA[name])
    g = synthetic.make_grid(kw.pop("nx"), kw.pop("ny"), kw.pop("nz"), **kw)
    return g, helpers.gridmetrics_of(g)


def pair(name, upwind=True):
    """test_kept_ops._pair, also for the grids of EXTRA (built here: helpers.CASES is other tests' list too and stays as it is)."""
    from test_kept_ops import _pair

    if name not in EXTRA:
        return _pair(name, upwind=upwind)
    import torch

    from otmb_amd.device import DeviceAssembler

    g, gm = grid(name)
    asms = []
    for _ in range(2):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=upwind)
        asms.append(a)
    asms[1]._kept_ops = lambda out: (0, ())
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    return g, gm, asms[0], asms[1], umo, vmo, g.umo.properties["_FillValue"]


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
    rec["kept_vrtab"] = asm.ctx.kept_vrtab()
    rec["kept_nbtab"] = asm.ctx.kept_nbtab()
    asm.ctx.timing_enable(False)
    return rec


def run_rho_nan_pipeline(steps=4):
    """A NaN ρ at a wet cell, then a `steps`-step asynchronous pipeline: (error text, failing step), every step's status and nnz."""
    from otmb_amd.capi import OtmbError
    from test_kept_ops import _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    asm.rho[wet_regular_cell(asm)] = float("nan")
    err = None
    try:
        for _ in range(steps):
            asm.step_async(umo, vmo, fill)
            # (every step after the first keeps and promises ρ: the first one's call was accepted, the NaN is found only when the pipeline is folded)
        asm.finish()
    except OtmbError as e:
        err = (str(e), e.step)
    return {"error": err, "steps": [list(asm.result_step(k)) for k in range(steps)]}


def main(path):
    res = {"cases": {f"{n}|{u}|{p}": run_case(n, u, p, with_full=False) for n, u, p in cases()}, "nan": run_rho_nan_pipeline()}
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
