"""CPU: the lane code of csrc/otmb_periodic.hip that needs no barrier (pd_dots_lane, pd_update_lane with the pair loads and stores under them,
pd_fold_kernel, pd_scale_kernel and pd_combine_kernel), text as it stands, compiled as plain C++ and executed lane by lane by a stand-alone host program under AddressSanitizer and
UBSan, on arrays of exactly the sizes the library's layout gives them (an even leading dimension, 16-byte aligned columns, NaN in the padding
row): every lane's accumulators, the folded sums and the updated vector have the bits of the restatement's order (tests/periodic_ref.py:
_lanes, _fold, device_update), the scaled vector those of w / s and the combined x those of the sequential x + Σ y_j·V_j, on an aligned x and
on one whose base is 8 bytes off a 16-byte boundary (alx false); no load is misaligned and nothing outside the arrays is touched.  The
workgroup's tree runs shuffles between barriers and cannot be run one lane at a time: the GPU tests (tests/test_periodic.py,
tests/test_periodic_rows.py) cover it."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import periodic_ref as PR
from test_step_host import PRELUDE, _definition, _hex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc", "otmb_periodic.hip")

VECTORS = r"""
#include <cstdlib>
struct alignas(16) double2 { double x, y; };
static inline double2 make_double2(double x, double y) { return double2{x, y}; }
"""

MAIN = r"""
template <class F> static void launch(i64 blocks, int bs, F f) {
    for (i64 b = 0; b < blocks; ++b)
        for (int t = 0; t < bs; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t; f(); }
}
static double *columns(i64 count) { return (double *)aligned_alloc(256, (size_t)((count * 8 + 255) / 256 * 256)); }  // (hipMalloc's alignment)
template <int NB, bool NORM> static void dots(i64 n, i64 np, const double *V, i64 ld, const double *w) {
    launch(np, 256, [&] {
        double acc[NB + 1];
        pd_dots_lane<NB, NORM>(n, V, ld, w, acc);
        for (int b = 0; b < NB + (NORM ? 1 : 0); ++b) printf("%a\n", acc[b]);
    });
}
static double *exactly(i64 count) {  // count doubles on a 256-byte base and not one more: the sanitizer sees a step too far
    void *p = nullptr;
    if (posix_memalign(&p, 256, (size_t)count * 8)) abort();
    return (double *)p;
}
// in: n, nj, np, nq; V (nj columns of ld = n rounded up to even), w (ld), h (nj), partials (nq x np), s, y (nj), x (ld)
// out: per register block of the basis (4, 2, 1; the first with ‖w‖²) and lane its accumulators; the folded partials; the updated w (n) and
//      the lanes' ‖w‖² accumulators; w / s (n); x + Σ y_j·V_j on the aligned x (n) and on the x one element into its buffer (n)
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long n, nj, np, nq;
    if (fscanf(f, "%lld %lld %lld %lld", &n, &nj, &np, &nq) != 4) return 2;
    const i64 ld = (n + 1) & ~(i64)1;
    double *V = columns(ld * nj), *w = columns(ld), *h = columns(nj), *part = columns(nq * np), *out = columns(nq);
    for (i64 i = 0; i < ld * nj; ++i) if (fscanf(f, "%la", V + i) != 1) return 2;
    for (i64 i = 0; i < ld; ++i) if (fscanf(f, "%la", w + i) != 1) return 2;
    for (i64 i = 0; i < nj; ++i) if (fscanf(f, "%la", h + i) != 1) return 2;
    for (i64 i = 0; i < nq * np; ++i) if (fscanf(f, "%la", part + i) != 1) return 2;
    double s, *y = columns(nj), *ws = exactly(ld), *xa = exactly(ld), *xbuf = exactly(n + 1), *xm = xbuf + 1;
    if (fscanf(f, "%la", &s) != 1) return 2;
    for (i64 i = 0; i < nj; ++i) if (fscanf(f, "%la", y + i) != 1) return 2;
    for (i64 i = 0; i < ld; ++i) if (fscanf(f, "%la", xa + i) != 1) return 2;
    for (i64 i = 0; i < ld; ++i) ws[i] = w[i];
    xbuf[0] = 7.25;
    for (i64 i = 0; i < n; ++i) xm[i] = xa[i];
    i64 j0 = 0;
    for (int nb : {4, 2, 1})  // op_blocks<PD_NB> over the basis
        for (; nj - j0 >= nb; j0 += nb) {
            const double *v = V + j0 * ld;
            if (nb == 4) { if (j0 == 0) dots<4, true>(n, np, v, ld, w); else dots<4, false>(n, np, v, ld, w); }
            if (nb == 2) { if (j0 == 0) dots<2, true>(n, np, v, ld, w); else dots<2, false>(n, np, v, ld, w); }
            if (nb == 1) { if (j0 == 0) dots<1, true>(n, np, v, ld, w); else dots<1, false>(n, np, v, ld, w); }
        }
    launch(1, 256, [&] { pd_fold_kernel(part, np, nq, out); });
    for (i64 q = 0; q < nq; ++q) printf("%a\n", out[q]);
    std::vector<double> acc((size_t)(np * 256));
    launch(np, 256, [&] { acc[(size_t)blockIdx.x * 256 + threadIdx.x] = pd_update_lane<true>(n, V, ld, nj, h, w); });
    for (i64 i = 0; i < n; ++i) printf("%a\n", w[i]);
    for (double a : acc) printf("%a\n", a);
    if (ld > n && w[n] == w[n]) return 3;  // the padding row was written
    launch(np, 256, [&] { pd_scale_kernel(n, ws, s); });
    for (i64 i = 0; i < n; ++i) printf("%a\n", ws[i]);
    if (ld > n && ws[n] == ws[n]) return 4;
    launch(np, 256, [&] { pd_combine_kernel(n, V, ld, nj, y, xa, true); });
    for (i64 i = 0; i < n; ++i) printf("%a\n", xa[i]);
    if (ld > n && xa[n] == xa[n]) return 5;
    if (((uintptr_t)xm & 15) != 8) return 6;  // (the case: an X that the 16-byte path must not take)
    launch(np, 256, [&] { pd_combine_kernel(n, V, ld, nj, y, xm, false); });
    for (i64 i = 0; i < n; ++i) printf("%a\n", xm[i]);
    if (xbuf[0] != 7.25) return 7;  // the element in front was written
    free(V), free(w), free(h), free(part), free(out), free(y), free(ws), free(xa), free(xbuf);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this host")
    src = open(SRC, encoding="utf-8").read()
    rows = re.search(r"^#define PD_ROWS \d+", src, re.M).group(0) + "\n"
    assert int(rows.split()[-1]) == PR.PD_ROWS
    code = "".join(_definition(src, name) for name in ("Pd2", "pd_load", "pd_store", "pd_row", "pd_dots_lane", "pd_fold_kernel", "pd_update_lane", "pd_combine_kernel", "pd_scale_kernel"))
    d = tmp_path_factory.mktemp("periodic_host")
    cpp, exe = str(d / "periodic_host.cpp"), str(d / "periodic_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(PRELUDE + VECTORS + rows + code + MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", exe, cpp], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr) and "error:" not in r.stderr:
        pytest.skip("g++ here has no static AddressSanitizer / UBSan runtime to link")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [1, 118, 512, 513, PR.PD_ROWS, PR.PD_ROWS + 1, 2 * PR.PD_ROWS + 513])
def test_dots_and_update_loops_as_host_code_have_the_bits_of_the_restatement(program, n):
    """n = 1 (one row, no pair), 118 (even: no padding row, one workgroup, lanes without rows), 512 (every lane one pair, none a second),
    513 (lane 0 a second pair of a single row), 2048 (one workgroup exactly full), 2049 (a second workgroup of one row beside the NaN
    padding), 4609 (odd, three workgroups, the last one partly filled, the last pair a single row beside the NaN padding); 7 basis vectors:
    register blocks 4 + 2 + 1.  pd_scale_kernel and pd_combine_kernel (no barrier, as pd_fold_kernel has none) run as whole kernels: w / s,
    and x + Σ y_j·V_j at alx true (an x of the library's layout) and false (an x one element into a buffer of n + 1)."""
    exe, path = program
    nj, nq = 7, 9
    nwg = (n + PR.PD_ROWS - 1) // PR.PD_ROWS
    ld = (n + 1) & ~1
    rng = np.random.default_rng(n)
    V, w, h = rng.standard_normal((nj, n)), rng.standard_normal(n), rng.standard_normal(nj)
    part = rng.standard_normal((nq, nwg))
    s, y, x = float(rng.uniform(0.5, 3.0)), rng.standard_normal(nj), rng.standard_normal(n)
    Vp, wp, xp = np.full((nj, ld), np.nan), np.full(ld, np.nan), np.full(ld, np.nan)  # the padding row must be neither read into a sum nor written
    Vp[:, :n], wp[:n], xp[:n] = V, w, x
    with open(path, "w") as f:
        f.write(f"{n} {nj} {nwg} {nq}\n{_hex(Vp.T)}\n{_hex(wp)}\n{_hex(h)}\n{_hex(part.T)}\n{_hex([s])}\n{_hex(y)}\n{_hex(xp)}\n")  # (_hex writes column-major: V_j contiguous)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])  # (a sanitizer report ends the program with a non-zero status)
    out = np.array([float.fromhex(x) for x in r.stdout.split()])
    at = 0
    j0 = 0
    for nb in (4, 2, 1):
        while nj - j0 >= nb:
            nv = nb + (1 if j0 == 0 else 0)
            got = out[at:at + nwg * 256 * nv].reshape(nwg, 256, nv)
            at += got.size
            for b in range(nb):
                assert np.array_equal(_bits(got[:, :, b]), _bits(PR._lanes(V[j0 + b] * w))), (n, "V_j·w", j0 + b)
            if j0 == 0:
                assert np.array_equal(_bits(got[:, :, nb]), _bits(PR._lanes(w * w))), (n, "‖w‖²")
            j0 += nb
    assert j0 == nj
    folded = out[at:at + nq]
    at += nq
    assert np.array_equal(_bits(folded), _bits([PR._fold(part[q]) for q in range(nq)])), (n, "fold")
    want = PR.device_update(V, h, w)
    assert np.array_equal(_bits(out[at:at + n]), _bits(want)), (n, "update")
    at += n
    assert np.array_equal(_bits(out[at:at + nwg * 256].reshape(nwg, 256)), _bits(PR._lanes(want * want))), (n, "‖w‖² of the update")
    at += nwg * 256
    assert np.array_equal(_bits(out[at:at + n]), _bits(w / s)), (n, "scale")
    at += n
    combined = x.copy()
    for j in range(nj):  # periodic_column's x += y_j·V_j
        combined = combined + y[j] * V[j]
    assert np.array_equal(_bits(out[at:at + n]), _bits(combined)), (n, "combine, alx")
    at += n
    assert np.array_equal(_bits(out[at:at + n]), _bits(combined)), (n, "combine, 8 bytes off")
    assert at + n == len(out)
