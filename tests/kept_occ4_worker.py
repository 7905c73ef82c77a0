"""Scenarios of tests/test_kept_occ4.py, importable and runnable as a child process: the switch of the lean kept fill (OTMB_KEPT_OCC4) is read
once per process, so the OTMB_KEPT_OCC4=0 side of every comparison (the three-wave instantiation) runs here and writes its digests to a JSON file.

    python tests/kept_occ4_worker.py OUT.json        (needs a GPU)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import helpers  # noqa: E402
from helpers import COUNTS_ON  # noqa: E402
import kept_vrtab_worker as W  # noqa: E402

KEPT = W.KEPT
# 436 wet columns: two tiles of 256; the second holds 180, so its third wave ends at lane 52 and its fourth is empty.  Columns at i = 0 and
# i = nx - 1 at every level of the northern rows (the periodic wrap orders), 74 on the seam row (tripolar: the generic builder, inside the
# lean kernel, in waves that also hold regular columns).  The same wet mask under both topologies.
BASE = dict(nx=40, ny=24, nz=6, land_fraction=0.93, seed=10, rho="array")
GRIDS = {"occ4_tripolar": dict(BASE, topology="tripolar"), "occ4_bipolar": dict(BASE, topology="bipolar")}
PROTOCOLS = ["async", "fused", "twophase"]


def grid(name):
    from otmb_amd import synthetic

    kw = dict(GRIDS[name])
    g = synthetic.make_grid(kw.pop("nx"), kw.pop("ny"), kw.pop("nz"), **kw)
    return g, helpers.gridmetrics_of(g)


def pair(name, upwind=True, kappa=None):
    """W.pair for its grids; the same two assemblers (one that promises, one that never does) for the grids of GRIDS."""
    if name not in GRIDS:
        assert kappa is None
        return W.pair(name, upwind=upwind)
    import torch

    from otmb_amd.device import DeviceAssembler

    g, gm = grid(name)
    kap = kappa or (g.kappaH, g.kappaVML, g.kappaVdeep)
    asms = []
    for _ in range(2):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, g.rho, *kap, upwind=upwind)
        asms.append(a)
    asms[1]._kept_ops = lambda out: (0, ())
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    return g, gm, asms[0], asms[1], umo, vmo, g.umo.properties["_FillValue"]


def own_cases():
    return [(n, u, p) for n in GRIDS for u in (True, False) for p in PROTOCOLS if p != "fused" or COUNTS_ON]


def run_case(name, upwind, protocol, steps=5, with_full=True, kappa=None, fields=None):
    """W.run_case, on the grids of GRIDS as well, with what otmb_ctx_kept_occ4 says after the last step."""
    from test_kept_ops import _fields, _run

    g, gm, asm, full, umo, vmo, fill = pair(name, upwind=upwind, kappa=kappa)
    rec = {"kept": [], "full": [], "kept_steps": [], "occ4_steps": []}
    for u, v in (fields or _fields)(umo, vmo, steps, seed=len(name)):
        _run(asm, protocol, u, v, fill)
        rec["kept"].append(W.digest(asm))
        if with_full:
            _run(full, protocol, u, v, fill)
            rec["full"].append(W.digest(full))
        rec["kept_steps"].append(asm._kept_last == KEPT)
        rec["occ4_steps"].append(asm.ctx.kept_occ4())
    rec["kept_occ4"] = asm.ctx.kept_occ4()
    rec["kept_vrtab"] = asm.ctx.kept_vrtab()
    return rec


def union_nnz(asm):
    """Entries T would hold if nothing cancelled: the union of the four operators' patterns."""
    from helpers import MATS

    keys = []
    for k, m in enumerate(MATS):
        if m == "T":
            continue
        cp = asm.out[m][0].cpu().numpy()
        rv = asm.out[m][1][: asm.nnz[k]].cpu().numpy()
        col = np.repeat(np.arange(asm.N, dtype=np.int64), np.diff(cp))
        keys.append(col * (asm.N + 1) + rv)
    return int(np.unique(np.concatenate(keys)).size)


def run_cancellation(name="occ4_tripolar", steps=4):
    """κ = 0 with centred weights: the diffusive values are explicit zeros, T's rows without a flux cancel exactly (FLAG_T_CANCEL: the step's T is
    compacted when it is folded).  Per step the digests, T's count against the union's, and which kernel filled."""
    from test_kept_ops import _fields, _run

    g, gm, asm, full, umo, vmo, fill = pair(name, upwind=False, kappa=(0.0, 0.0, 0.0))
    rec = {"kept": [], "full": [], "nnzT": [], "union": [], "kept_steps": [], "occ4_steps": []}
    for u, v in _fields(umo, vmo, steps, seed=3):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        rec["kept"].append(W.digest(asm))
        rec["full"].append(W.digest(full))
        rec["nnzT"].append(asm.nnz[0])
        rec["union"].append(union_nnz(asm))
        rec["kept_steps"].append(asm._kept_last == KEPT)
        rec["occ4_steps"].append(asm.ctx.kept_occ4())
    return rec


def run_capacity(name="occ4_tripolar"):
    """Two steps on the same fields (the second keeps), then the same step again into arrays whose Tadv capacity is one entry short."""
    from otmb_amd.capi import OtmbError
    from test_kept_ops import _run

    g, gm, asm, full, umo, vmo, fill = pair(name)
    for _ in range(2):
        _run(asm, "async", umo, vmo, fill)
    assert asm._kept_last == KEPT
    caps = list(asm._capacities())
    caps[1] = asm.nnz[1] - 1
    asm._capacities = lambda: caps
    err = None
    try:
        _run(asm, "async", umo, vmo, fill)
    except OtmbError as e:
        err = [e.status, str(e), e.step]
    return {"error": err, "occ4": asm.ctx.kept_occ4(), "vrtab": asm.ctx.kept_vrtab(), "steps": [list(asm.result_step(0))]}


def main(path):
    res = {"cases": {f"{n}|{u}|{p}": run_case(n, u, p, with_full=False) for n, u, p in W.cases() + own_cases()},
           "cancel": run_cancellation(), "capacity": run_capacity(), "nan": W.run_rho_nan_pipeline()}
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
