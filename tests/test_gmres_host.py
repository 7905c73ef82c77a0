"""CPU: the least-squares problem of a GMRES column (csrc/otmb_gmres.h: GmresLsq's start, push and solve, the host arithmetic that decides
when csrc/otmb_periodic.hip accepts, restarts or stops a column), the header as it stands, driven by a stand-alone host program under
AddressSanitizer and UBSan: after every push the rotation, the triangle's diagonal entry, the rotated right-hand side, the recursive
residual and the y of the back substitution have the BITS of the restatement -- tests/periodic_ref.py's givens_column, which periodic_column
itself calls, and its back_substitution, term by term in C's order (numpy's `@` adds in another order and does not agree), which
periodic_column calls in its device order."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import periodic_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include <cstring>

#include "otmb_gmres.h"

static void bits(double x) {
    unsigned long long u;
    memcpy(&u, &x, 8);
    printf("%016llx\n", u);
}
// in: m, beta, the number of columns, then per column h1 and h2 (i + 2 hex floats each, i the record's own count of accepted columns)
// out: per column "push 0 <i>" (refused) or "push 1 <i>" and the bits of cs[i-1], sn[i-1], R(i-1, i-1), gv[i], est and y[0..i)
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long m, ncols;
    double beta;
    if (!f || fscanf(f, "%lld %la %lld", &m, &beta, &ncols) != 3) return 2;
    GmresLsq ls;
    ls.start(m, beta);
    for (long long c = 0; c < ncols; ++c) {
        std::vector<double> h1((size_t)(ls.i + 2)), h2((size_t)(ls.i + 2)), y((size_t)(ls.i + 1));  // (exact sizes: the sanitizer sees a step too far)
        for (auto &v : h1) if (fscanf(f, "%la", &v) != 1) return 2;
        for (auto &v : h2) if (fscanf(f, "%la", &v) != 1) return 2;
        double hn = -1.0, est = -1.0;
        const bool ok = ls.push(h1.data(), h2.data(), &hn, &est);
        printf("push %d %lld\n", (int)ok, (long long)ls.i);
        if (!ok) continue;
        const int64_t i = ls.i - 1;
        bits(ls.cs[(size_t)i]), bits(ls.sn[(size_t)i]), bits(ls.R[(size_t)(i * (m + 1) + i)]), bits(ls.gv[(size_t)(i + 1)]), bits(est);
        ls.solve(y.data());
        for (double v : y) bits(v);
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this host")
    d = tmp_path_factory.mktemp("gmres_host")
    cpp, exe = str(d / "gmres_host.cpp"), str(d / "gmres_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, cpp], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr) and "error:" not in r.stderr:
        pytest.skip("g++ here has no static AddressSanitizer / UBSan runtime to link")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _bits(a):
    return [int(x) for x in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


def _restated(m, beta, cols):
    """Per column None (refused: an input is not finite) or the bits the program prints.  cols: (h1, h2) of i + 2 entries each, i the number
    of columns accepted before."""
    Rm, cs, sn, gv = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
    gv[0] = beta
    i, out = 0, []
    with np.errstate(all="ignore"):  # (the rr = 0 column divides by zero on purpose)
        for h1, h2 in cols:
            assert len(h1) == len(h2) == i + 2
            h = h1[:i + 1] + h2[:i + 1]
            if not (np.isfinite(h1[i + 1]) and np.isfinite(h2[i + 1]) and np.isfinite(h).all()):
                out.append(None)
                continue
            hn = np.sqrt(h2[i + 1])
            PR.givens_column(h, hn, cs, sn, gv, i)
            Rm[:i + 1, i] = h
            i += 1
            y = PR.back_substitution(Rm, gv, i)  # C's order: s = s - R·y[b], b ascending, then the division
            out.append(_bits([cs[i - 1], sn[i - 1], Rm[i - 1, i - 1], gv[i], np.abs(gv[i])]) + _bits(y))
    return out


def _run(program, m, beta, cols):
    """-> per column None or the printed bits, with the count of accepted columns the program reports checked on the way"""
    exe, path = program
    with open(path, "w") as f:
        f.write(f"{m} {float(beta).hex()} {len(cols)}\n")
        for h1, h2 in cols:
            f.write(" ".join(float(x).hex() for x in h1) + "\n" + " ".join(float(x).hex() for x in h2) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])  # (a sanitizer report ends the program with a non-zero status)
    out, accepted = [], 0
    lines = r.stdout.split("\n")
    at = 0
    for _ in cols:
        word, ok, i = lines[at].split()
        at += 1
        assert word == "push"
        accepted += int(ok)
        assert int(i) == accepted  # (a refused column leaves i where it stood)
        if ok == "0":
            out.append(None)
            continue
        out.append([int(x, 16) for x in lines[at:at + 5 + accepted]])
        at += 5 + accepted
    assert lines[at:] == [""]
    return out


def _columns(rng, count, first=0):
    """Random columns first..first + count - 1, every entry scaled by its own power of ten over 1e-8 .. 1e2; ‖w‖² is a square."""
    cols = []
    for i in range(first, first + count):
        h1 = rng.standard_normal(i + 2) * 10.0 ** rng.uniform(-8, 2, i + 2)
        h2 = rng.standard_normal(i + 2) * 10.0 ** rng.uniform(-8, 2, i + 2)
        h1[i + 1], h2[i + 1] = h1[i + 1] ** 2, h2[i + 1] ** 2  # (the first pass's ‖w‖² slot is read for finiteness only)
        cols.append((h1, h2))
    return cols


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("m", [1, 5, 30])
def test_push_and_solve_have_the_bits_of_the_restatement(program, m, seed):
    rng = np.random.default_rng(100 * m + seed)
    cols = _columns(rng, m)
    beta = float(abs(rng.standard_normal()) * 10.0 ** rng.uniform(-8, 2))
    got, want = _run(program, m, beta, cols), _restated(m, beta, cols)
    assert all(w is not None for w in want)
    assert got == want


@pytest.mark.parametrize("m,at", [(1, 0), (5, 2), (5, 4)])
def test_a_column_that_ends_the_krylov_space(program, m, at):
    """‖w‖² = 0 beside an h that is not zero: sn = 0 and |cs| = 1; and h = 0 with ‖w‖² = 0, the rr = 0 branch: cs = 1, sn = 0, a zero on
    the triangle's diagonal, so y holds infinities and NaN -- the same ones, bit for bit."""
    rng = np.random.default_rng(7 + at)
    head = _columns(rng, at)
    one = _columns(rng, 1, first=at)[0]
    one[1][at + 1] = 0.0
    got, want = _run(program, m, 0.75, head + [one]), _restated(m, 0.75, head + [one])
    assert got == want and want[-1] is not None
    assert want[-1][1] == _bits([0.0])[0] and want[-1][0] in (_bits([1.0])[0], _bits([-1.0])[0])  # sn = +0.0, cs = ±1
    zero = (np.zeros(at + 2), np.zeros(at + 2))
    got, want = _run(program, m, 0.75, head + [zero]), _restated(m, 0.75, head + [zero])
    assert got == want and want[-1] is not None
    assert want[-1][:3] == _bits([1.0, 0.0, 0.0])  # cs = 1, sn = 0, R(i, i) = 0
    assert not np.isfinite(np.array(want[-1][5:], dtype=np.uint64).view(np.float64)).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", ["h1[0]", "h1[i]", "h2[0]", "h2[i]", "h1[i + 1]", "h2[i + 1]"])
def test_a_nonfinite_input_is_refused(program, where, bad):
    """A NaN or an infinity in h', in h'' and in either ‖w‖² slot: push returns false and i stands; the finite column that follows is
    taken as if nothing had been offered before it."""
    m, at = 5, 2
    rng = np.random.default_rng(11)
    head = _columns(rng, at)
    spoilt, clean = _columns(rng, 1, first=at)[0], _columns(rng, 1, first=at)[0]
    which, index = where[:2], {"0": 0, "i": at, "i + 1": at + 1}[where[3:-1]]
    spoilt[0 if which == "h1" else 1][index] = bad
    cols = head + [spoilt, clean]
    got, want = _run(program, m, 3.5, cols), _restated(m, 3.5, cols)
    assert want[at] is None and want[at + 1] is not None
    assert got == want
    assert got[at + 1] == _run(program, m, 3.5, head + [clean])[at]
