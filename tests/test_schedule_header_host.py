"""CPU: the schedule of a stepped cycle (csrc/otmb_sched.h: StSched's at, weights, blocks, mean_weights and describe, and the complaints of
the scheduled calls -- the host arithmetic that decides which slot a step of csrc/otmb_step.hip takes, whether it blends, how many
preconditioner blocks a call reserves and what csrc/otmb_periodic.hip's cycle-mean weighs), the header as it stands, driven by a
stand-alone host program under AddressSanitizer and UBSan.  What it prints is compared with the restatements the GPU tests own:
tests/sched_ref.py (slot_of, visit_weights), tests/interp_ref.py (kind, combine_weights, mean_weights, prec_blocks) and
tests/periodic_pc_ref.py (visit_weights); tests/season_ref.py's field picks its blocks by interp_ref.kind, the rule checked here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import interp_ref as IR
import periodic_pc_ref as PC
import sched_ref as SC
import season_ref as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc")
NSLOTS = 3

MAIN = r"""
#include <cstring>

#include "otmb_sched.h"

static void bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    printf(" %016llx", u);
}
// the arrays are of the exact sizes the header may read: the sanitizer sees a step too far
struct Lists {
    std::vector<int64_t> a, b;
    std::vector<double> w;
    bool read(FILE *f, long long count) {
        a.resize((size_t)count), b.resize((size_t)count), w.resize((size_t)count);
        for (auto *v : {&a, &b})
            for (auto &x : *v) {
                long long y;
                if (fscanf(f, "%lld", &y) != 1) return false;
                x = y;
            }
        for (auto &x : w)
            if (fscanf(f, "%la", &x) != 1) return false;
        return true;
    }
};
// mode 0: no array; 1: `count` blocks; 2: the same with block 1 null
static const double *const *blocks_of(int mode, long long count, std::vector<const double *> &keep) {
    static const double cell = 0.0;
    keep.assign((size_t)(count > 0 ? count : 0), &cell);
    if (mode == 2 && count > 1) keep[1] = nullptr;
    return mode == 0 ? nullptr : keep.data();
}
// in: nslots, then records
//   c first_slot substeps nsteps            a cyclic schedule
//   x nsteps a.. b.. w..                    a listed one (hex floats)
//   S n substeps nsrc mode lds              sv_sched_complaint
//   I n per_slot nsrc mode lds nulls count a.. b.. w..   sv_interp_complaint (nulls: the three arrays are not given)
//   D n nd mode ldd                         sv_season_complaint
// out: per schedule "steps <nsteps>", per step "<slot> <blend>[ wa wb bits]|<describe>", "blocks <used> <blended>", "mean <bits>.." (nsteps > 0);
//      per complaint "says <text>" or "says nothing"
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long nslots;
    if (!f || fscanf(f, "%lld", &nslots) != 1) return 2;
    char kind[4];
    while (fscanf(f, "%3s", kind) == 1) {
        if (kind[0] == 'c' || kind[0] == 'x') {
            long long first = 0, substeps = 1, nsteps;
            Lists l;
            if (kind[0] == 'c' ? fscanf(f, "%lld %lld %lld", &first, &substeps, &nsteps) != 3 : (fscanf(f, "%lld", &nsteps) != 1 || !l.read(f, nsteps))) return 2;
            const StSched s = kind[0] == 'c' ? StSched::cyclic(first, substeps) : StSched::list(l.a.data(), l.b.data(), l.w.data());
            printf("steps %lld\n", nsteps);
            for (long long t = 0; t < nsteps; ++t) {
                const StStep at = s.at(t, nslots);
                printf("%lld %d", (long long)at.slot, (int)at.blend);
                if (at.blend) {
                    double wa = -1.0, wb = -1.0;
                    s.weights(t, wa, wb);
                    bits(wa), bits(wb);
                }
                printf("|%s\n", s.describe(t, at.slot).c_str());
            }
            bool blended = false;
            const long long used = s.blocks(nsteps, nslots, blended);
            printf("blocks %lld %d\n", used, (int)blended);
            if (nsteps > 0) {
                std::vector<double> wt((size_t)nslots, -1.0);
                s.mean_weights(nsteps, nslots, wt.data());
                printf("mean");
                for (double v : wt) bits(v);
                printf("\n");
            }
            continue;
        }
        long long n, p[6];
        std::vector<const double *> keep;
        const char *says = nullptr;
        char text[160];
        Lists l;
        if (kind[0] == 'S') {
            if (fscanf(f, "%lld %lld %lld %lld %lld", &n, &p[0], &p[1], &p[2], &p[3]) != 5) return 2;
            says = sv_sched_complaint(n, nslots, p[0], p[1], blocks_of((int)p[2], p[1], keep), p[3]);
        } else if (kind[0] == 'I') {
            if (fscanf(f, "%lld %lld %lld %lld %lld %lld %lld", &n, &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) != 7 || !l.read(f, p[4] ? 0 : p[5])) return 2;
            const StMix mix = p[4] ? StMix{nullptr, nullptr, nullptr} : StMix{l.a.data(), l.b.data(), l.w.data()};
            says = sv_interp_complaint(n, nslots, p[5], mix, p[1], blocks_of((int)p[2], p[1], keep), p[3], text, p[0] != 0);
        } else if (kind[0] == 'D') {
            if (fscanf(f, "%lld %lld %lld %lld", &n, &p[0], &p[1], &p[2]) != 4) return 2;
            says = sv_season_complaint(n, nslots, p[0], blocks_of((int)p[1], p[0], keep), p[2]);
        } else {
            return 2;
        }
        printf("says %s\n", says ? says : "nothing");
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this host")
    d = tmp_path_factory.mktemp("sched_host")
    cpp, exe = str(d / "sched_host.cpp"), str(d / "sched_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, cpp], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr) and "error:" not in r.stderr:
        pytest.skip("g++ here has no static AddressSanitizer / UBSan runtime to link")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


def _lists(a, b, w):
    return " ".join(str(int(x)) for x in list(a) + list(b)) + " " + " ".join(float(x).hex() for x in w)


def _run(program, records):
    exe, path = program
    with open(path, "w") as f:
        f.write(f"{NSLOTS}\n" + "\n".join(records) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])  # (a sanitizer report ends the program with a non-zero status)
    return r.stdout.split("\n")


def _schedule(program, record, nsteps):
    """-> (per step (slot, blend, [wa, wb bits] or [], describe), (used, blended), the mean's bits or None)"""
    lines = _run(program, [record])
    assert lines[0] == f"steps {nsteps}"
    steps = []
    for line in lines[1:1 + nsteps]:
        head, text = line.split("|", 1)
        slot, blend, *w = head.split()
        steps.append((int(slot), bool(int(blend)), [int(x, 16) for x in w], text))
    used, blended = lines[1 + nsteps].split()[1:]
    assert lines[1 + nsteps].startswith("blocks ")
    rest = lines[2 + nsteps:]
    mean = None
    if nsteps > 0:
        assert rest[0].startswith("mean ")
        mean, rest = [int(x, 16) for x in rest[0].split()[1:]], rest[1:]
    assert rest == [""]
    return steps, (int(used), bool(int(blended))), mean


@pytest.mark.parametrize("nsteps", [0, 1, 7])
@pytest.mark.parametrize("substeps", [1, 2, 5, 9])  # (9: more sub-steps than the call has steps)
def test_a_cyclic_schedule(program, substeps, nsteps):
    first = 2
    steps, blocks, mean = _schedule(program, f"c {first} {substeps} {nsteps}", nsteps)
    slots = [SC.slot_of(t, first, substeps, NSLOTS) for t in range(nsteps)]
    assert steps == [(s, False, [], f" (step {t}, slot {s})") for t, s in enumerate(slots)]
    assert blocks == (IR.prec_blocks([("plain", s) for s in slots]), False)
    if nsteps > 0:
        assert mean == _bits(SC.visit_weights(NSLOTS, nsteps, first, substeps))
        count = [slots.count(s) for s in range(NSLOTS)]
        assert mean == _bits([c / nsteps for c in count])  # the accumulator of doubles only ever added 1.0: the bits of count / ncycle
        if substeps == 1:
            assert mean == _bits(PC.visit_weights(NSLOTS, nsteps, first))


LISTED = {
    "a == b, whatever the weight": ([1, 1, 2, 2], [1, 1, 2, 2], [0.0, 1.0, 0.25, 0.5]),
    "w = 0, 1 and 0.25": ([0, 0, 0, 2, 2], [1, 1, 1, 0, 0], [0.0, 1.0, 0.25, 1.0, 0.0]),
    "only blended steps": ([0, 1, 2, 0], [1, 2, 0, 2], [0.25, 0.5, 0.1, 0.75]),
    "only plain steps on one slot": ([1, 1, 0, 1], [1, 2, 1, 1], [0.5, 0.0, 1.0, 0.25]),
    "slot 2 is never visited": ([0, 1, 0, 1, 0], [1, 0, 0, 1, 1], [0.25, 0.3, 0.0, 1.0, 1.0]),
    "one step": ([2], [0], [0.625]),
    "no step": ([], [], []),
}


@pytest.mark.parametrize("name", list(LISTED))
def test_a_listed_schedule(program, name):
    a, b, w = LISTED[name]
    nsteps = len(w)
    steps, blocks, mean = _schedule(program, f"x {nsteps} " + _lists(a, b, w), nsteps)
    kinds = [IR.kind(x, y, z) for x, y, z in zip(a, b, w)]
    want = []
    for t, (what, slot) in enumerate(kinds):
        wt = IR.combine_weights(NSLOTS, a[t], b[t], w[t])
        text = f" (step {t}, slots {a[t]} and {b[t]}, weight {'%.17g' % w[t]})"
        want.append((slot, False, [], text) if what == "plain" else (a[t], True, _bits([wt[a[t]], wt[b[t]]]), text))
    assert steps == want
    assert blocks == (IR.prec_blocks(kinds), any(what == "blend" for what, _ in kinds))
    if nsteps > 0:
        assert mean == _bits(IR.mean_weights(NSLOTS, a, b, w))
    # season_ref picks a per-slot field's block by the same rule: the slot's own on a plain step, the two slots' fold on a blended one
    field = [np.full(2, 10.0 + s) for s in range(NSLOTS)]
    for t, (what, slot) in enumerate(kinds):
        got = SE.field(field, a[t], b[t], w[t])
        assert (got is field[steps[t][0]]) == (not steps[t][1])
    if name == "only plain steps on one slot":
        assert {s for s, _, _, _ in steps} == {1} and blocks == (1, False)
    if name == "only blended steps":
        assert blocks == (1, True)
    if name == "slot 2 is never visited":
        assert mean[2] == _bits([0.0])[0]  # +0.0, not -0.0


OK_LISTS = ([0, 1, 2, 0], [1, 2, 0, 0], [0.5, 0.25, 0.0, 1.0])


def _interp(n=5, per_slot=0, nsrc=1, mode=1, lds=5, nulls=0, lists=OK_LISTS):
    return f"I {n} {per_slot} {nsrc} {mode} {lds} {nulls} {len(lists[2])} " + ("" if nulls else _lists(*lists))


def test_what_the_scheduled_calls_refuse(program):
    nsrc_text, nd_text = "nsrc must be 0, 1 or the number of slots", "nd must be 0, 1 or the number of slots"
    ldd_text = "ldd must be 0 (the n values of a block serve every column) or >= n"
    a, b, w = OK_LISTS
    cases = [
        ("S 5 1 0 0 0", None), ("S 5 2 1 1 5", None), ("S 5 1 3 1 7", None), ("S 5 0 1 1 5", "substeps must be >= 1"), ("S 5 -3 0 0 5", "substeps must be >= 1"),
        ("S 5 1 2 1 5", nsrc_text), ("S 5 1 -1 1 5", nsrc_text), ("S 5 1 1 0 5", "S is null with nsrc > 0"), ("S 5 1 3 2 5", "a source block is null"),
        ("S 5 1 1 1 4", "lds is smaller than the rows of S"), ("S 5 1 0 0 4", None),
        (_interp(), None), (_interp(nsrc=0, mode=0), None), (_interp(per_slot=1, nsrc=3), None), (_interp(lists=([], [], [])), None),
        (_interp(nsrc=3), "nsrc must be 0 or 1 (a source per slot is not built with interpolation)"),
        (_interp(nsrc=2), "nsrc must be 0 or 1 (a source per slot is not built with interpolation)"), (_interp(per_slot=1, nsrc=2), nsrc_text),
        (_interp(mode=0), "S is null with nsrc > 0"), (_interp(per_slot=1, nsrc=3, mode=2), "a source block is null"),
        (_interp(lds=4), "lds is smaller than the rows of S"), (_interp(nulls=1), "slot_a, slot_b or weight is null"),
        (_interp(lists=([0, 1, 3, 0], b, w)), "step 2: slot 3 is outside 0..2 (otmb_op_set_slots)"),
        (_interp(lists=(a, [-1, 2, 0, 0], w)), "step 0: slot -1 is outside 0..2 (otmb_op_set_slots)"),
        (_interp(lists=(a, b, [0.5, np.nan, 0.0, 1.0])), "step 1: the weight nan is not finite or outside [0, 1]"),
        (_interp(lists=(a, b, [0.5, 0.25, 1.5, 1.0])), "step 2: the weight 1.5 is not finite or outside [0, 1]"),
        (_interp(lists=(a, b, [0.5, 0.25, 0.0, np.inf])), "step 3: the weight inf is not finite or outside [0, 1]"),
        (_interp(lists=(a, b, [-0.25, 0.25, 0.0, 1.0])), "step 0: the weight -0.25 is not finite or outside [0, 1]"),
        ("D 5 0 0 0", None), ("D 5 1 1 0", None), ("D 5 3 1 5", None), ("D 5 3 1 8", None), ("D 5 2 1 0", nd_text), ("D 5 -1 1 0", nd_text),
        ("D 5 1 0 0", "D is null with nd > 0"), ("D 5 3 2 0", "a d block is null"), ("D 5 3 1 4", ldd_text), ("D 5 1 1 1", ldd_text),
    ]
    lines = _run(program, [record for record, _ in cases])
    assert lines == ["says nothing" if text is None else "says " + text for _, text in cases] + [""]
