"""The kept-step sequence of tests/test_mid_grids.py, importable and runnable as a child process: the kept fill's switches (OTMB_KEPT_NBTAB,
OTMB_KEPT_HTAB, OTMB_KEPT_VRTAB, OTMB_KEPT_TPAT; csrc/otmb_tm_kept.hip) are read once per process, so the run with one of them at its non-default
value happens here, in a fresh process and Context, against the oracle, and writes what the context reported to a JSON file.

    python tests/mid_grids_worker.py OUT.json        (needs a GPU; the switch comes with the environment)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mid_grids as mg  # noqa: E402
from helpers import COUNTS_ON, MATS, assert_csc_equal  # noqa: E402

KEPT = ("TκH", "TκVML", "TκVdeep")
PROTOCOLS = ["async", "pipeline", "fused", "twophase"]
STEPS = ("step0", "step1", "step2")


def dev(a):
    """A host array in column-major order as a flat device tensor."""
    import torch

    return torch.from_numpy(np.array(a, order="F", copy=True).ravel(order="F")).cuda()


def assembler(name, rho="array", kap="grid", upwind=True):
    from otmb_amd.device import DeviceAssembler

    g, gm = mg.case(name)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, mg.rho_of(name, rho), *mg.kappa(name, kap), upwind=upwind)
    return asm


def assert_matrices(asm, ref, what, mats=MATS):
    got = asm.result_to_host()
    for m in mats:
        assert_csc_equal(got[m], ref[m], f"{what}: {m}")
    return got


def kept_sequence(oracle, protocol, name="mid"):
    """Three different fields in sequence on one assembler: every step's five matrices are the oracle's for that field.  Returns which steps kept
    the three operators, what otmb_ctx_kept_t_pattern and otmb_ctx_tm_infill said after each, and the tables the last kept fill read.  One
    assembler (one Context) at a time: it is released before the function returns."""
    from test_kept_ops import _run

    asm = assembler(name)
    rec = {"kept": [], "tpat": [], "infill": [], "infill_groups": asm.ctx.tm_infill_groups()}
    for which in STEPS:
        u, v, fill = mg.field(name, which)
        _run(asm, protocol, dev(u), dev(v), fill)
        assert_matrices(asm, mg.reference(oracle, name, which), f"{name}/{protocol}/{which}")
        rec["kept"].append(asm._kept_last == KEPT)
        rec["tpat"].append(asm.ctx.kept_t_pattern())
        rec["infill"].append(asm.ctx.tm_infill())
    rec["tables"] = {"htab": asm.ctx.kept_htab(), "nbtab": asm.ctx.kept_nbtab(), "vrtab": asm.ctx.kept_vrtab()}
    asm.ctx.synchronize()
    del asm
    return rec


def check_kept_record(rec, protocol, tpat_on=True):
    """From the second step on every step keeps (two-phase: at least once -- a T or Tadv that outgrew its arrays is allocated anew and written in
    full), and T's pattern is kept where tests/test_kept_t_pattern.py expects it: every step after the first, two-phase wherever a step kept."""
    if protocol == "twophase":
        assert any(rec["kept"]), rec
    else:
        assert rec["kept"][1:] == [True] * (len(STEPS) - 1), rec
    for k, (kept, tpat) in enumerate(zip(rec["kept"], rec["tpat"])):
        if (k > 0 and protocol != "twophase") or (protocol == "twophase" and kept):
            assert tpat == (1 if tpat_on else 0), (protocol, k, rec)


def main(path):
    from oracle import oracle

    oracle.build()
    res = {p: kept_sequence(oracle, p) for p in PROTOCOLS if p != "fused" or COUNTS_ON}
    with open(path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main(sys.argv[1])
