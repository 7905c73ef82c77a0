"""Scenarios of tests/test_kept_htab.py, importable and runnable as a child process: the TκH table switch (OTMB_KEPT_HTAB) is read once per
process, so the fallback side of every comparison runs here with OTMB_KEPT_HTAB=0 and writes its digests to a JSON file.

    python tests/kept_htab_worker.py OUT.json        (needs a GPU)"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import COUNTS_ON, MATS  # noqa: E402

NAMES = ["tiny_tripolar", "tiny_rho3d", "odd_nx_fold", "even_fold_open", "small_rho3d", "float32_flux"]
PROTOCOLS = ["async", "pipeline", "fused", "twophase"]
KEPT = ("TκH", "TκVML", "TκVdeep")


def cases():
    return [(n, u, p) for n in NAMES for u in (True, False) for p in PROTOCOLS if p != "fused" or COUNTS_ON]


def digest(asm, out=None):
    """sha256 of every output array at its length, and nnz."""
    asm.ctx.synchronize()
    out = asm.out if out is None else out
    h = {}
    for k, m in enumerate(MATS):
        cp, rv, nz = out[m]
        n = asm.nnz[k]
        h[m] = [hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
                for a in (cp.cpu().numpy(), rv[:n].cpu().numpy(), nz[:n].cpu().numpy())]
    return {"arrays": h, "nnz": list(asm.nnz)}


def launches(asm):
    """{kernel name: launches} since the previous collect (the context's HIP-event timing must be on)."""
    return {k: v[1] for k, v in asm.ctx.timing_collect().items()}


def run_case(name, upwind, protocol, steps=5):
    """The kept assembler and one that never promises, over `steps` flux fields: per step the digests of both, and which steps kept."""
    from test_kept_ops import _fields, _pair, _run

    g, gm, asm, full, umo, vmo, fill = _pair(name, upwind=upwind)
    asm.ctx.timing_enable(True)
    rec = {"kept": [], "full": [], "kept_steps": []}
    for u, v in _fields(umo, vmo, steps, seed=len(name)):
        _run(asm, protocol, u, v, fill)
        _run(full, protocol, u, v, fill)
        rec["kept"].append(digest(asm))
        rec["full"].append(digest(full))
        rec["kept_steps"].append(asm._kept_last == KEPT)
    rec["launches"] = launches(asm)
    rec["kept_htab"] = asm.ctx.kept_htab()
    asm.ctx.timing_enable(False)
    return rec


def wet_regular_cell(asm):
    """Linear index of a wet cell off the first and last rows whose four horizontal neighbours are wet (its TκH columns are regular)."""
    lw = asm.lwet3d.cpu().numpy()
    nx, ny = asm.nx, asm.ny
    for L in asm.lwet[: asm.N].cpu().numpy() - 1:
        i, j = L % nx, (L // nx) % ny
        if 0 < j < ny - 1 and all(lw[x] != 0 for x in (L - nx, L + nx, L - i + (i + 1) % nx, L - i + (i - 1) % nx)):
            return int(L)
    raise AssertionError("no regular wet cell")


def run_nan_pipeline(steps=4):
    """A NaN thkcello at a wet cell, then a `steps`-step asynchronous pipeline: (error text, failing step, every step's status and nnz)."""
    from otmb_amd.capi import OtmbError
    from test_kept_ops import _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    asm.thk[wet_regular_cell(asm)] = float("nan")
    err = None
    try:
        for _ in range(steps):
            asm.step_async(umo, vmo, fill)
            # (every step after the first keeps: the first one's call was accepted, the NaN is found only when the pipeline is folded)
        asm.finish()
    except OtmbError as e:
        err = (str(e), e.step)
    return {"error": err, "steps": [list(asm.result_step(k)) for k in range(steps)]}


def main(path):
    res = {"cases": {f"{n}|{u}|{p}": run_case(n, u, p) for n, u, p in cases()}, "nan": run_nan_pipeline()}
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
