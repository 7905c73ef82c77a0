"""CPU: the right-hand side's streaming kernel (θ = 1) and short-row kernel (θ < 1, A) of csrc/otmb_step.hip, text as it stands with the
slice-row walk of csrc/otmb_op_fold.h, compiled as plain C++ and executed lane by lane by a stand-alone host program under AddressSanitizer
and UBSan, on arrays of exactly the sizes the library allocates and with leading dimensions above n: they give the bits of the numpy
restatement (tests/step_ref.py: rhs over tests/spmv_ref.py's product) and touch nothing outside their arrays.  The long-row and the Aᵀ
kernels stage through LDS between barriers and cannot be run one lane at a time: the GPU tests (tests/test_step.py) cover them."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solve_ref as R
import step_ref as SR
from spmv_ref import spmv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc")
N0 = 257

PRELUDE = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef int64_t i64;
#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct Dim { unsigned x; };
static Dim blockIdx, threadIdx;
"""

MAIN = r"""
template <class F> static void launch(i64 blocks, int bs, F f) {
    for (i64 b = 0; b < blocks; ++b)
        for (int t = 0; t < bs; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t; f(); }
}
// in: n, entries of the slices, slices, k, has d, has S, sigma, theta, c; val, col, elen, sbase, d, X (ld n + 2), S (ld n + 3); out: B
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long n, total, ns;
    int k, hasd, hass;
    double sigma, theta, c;
    if (fscanf(f, "%lld %lld %lld %d %d %d %la %la %la", &n, &total, &ns, &k, &hasd, &hass, &sigma, &theta, &c) != 9) return 2;
    std::vector<double> val(total), d(n), X((size_t)(n + 2) * k), S((size_t)(n + 3) * k), B((size_t)n * k, 7.25);
    std::vector<int> col(total), elen(n);
    std::vector<i64> sbase(ns + 1);
    for (auto &v : val) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : col) if (fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : elen) if (fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : sbase) { long long x; if (fscanf(f, "%lld", &x) != 1) return 2; v = x; }
    for (auto &v : d) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : X) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : S) if (fscanf(f, "%la", &v) != 1) return 2;
    StLine q = {sigma, theta, c};
    const double *dp = hasd ? d.data() : nullptr, *sp = hass ? S.data() : nullptr;
    int c0 = 0;
    for (int kb : {4, 2, 1})  // op_blocks<SV_KB>
        for (; k - c0 >= kb; c0 += kb) {
            const double *x = X.data() + (size_t)c0 * (n + 2), *s = sp ? sp + (size_t)c0 * (n + 3) : nullptr;
            double *b = B.data() + (size_t)c0 * n;
            launch((n + 255) / 256, 256, [&] {
                if (theta == 1.0) {
                    if (kb == 4) st_stream_kernel<4>(n, sigma, x, n + 2, s, n + 3, b, n);
                    if (kb == 2) st_stream_kernel<2>(n, sigma, x, n + 2, s, n + 3, b, n);
                    if (kb == 1) st_stream_kernel<1>(n, sigma, x, n + 2, s, n + 3, b, n);
                } else {
                    if (kb == 4) st_rows_kernel<4>(q, val.data(), col.data(), sbase.data(), elen.data(), n, dp, x, n + 2, s, n + 3, b, n);
                    if (kb == 2) st_rows_kernel<2>(q, val.data(), col.data(), sbase.data(), elen.data(), n, dp, x, n + 2, s, n + 3, b, n);
                    if (kb == 1) st_rows_kernel<1>(q, val.data(), col.data(), sbase.data(), elen.data(), n, dp, x, n + 2, s, n + 3, b, n);
                }
            });
        }
    for (double v : B) printf("%a\n", v);
    return 0;
}
"""


def _definition(text, name):
    """The definition of the struct or function `name`, cut by the code's own tokens: from the line that introduces it (with a
    `template <...>` line before it, if there is one) to the brace that closes its body (and a struct's semicolon)."""
    m = re.search(r"^(?:template <[^\n]*>\n)?[^\n;/]*\b" + re.escape(name) + r"\b[^;]*?\{", text, re.M)
    assert m, name
    depth, j = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[m.start():j] + (";" if text[j:j + 1] == ";" else "") + "\n"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this host")
    step = open(os.path.join(CSRC, "otmb_step.hip"), encoding="utf-8").read()
    fold = open(os.path.join(CSRC, "otmb_op_fold.h"), encoding="utf-8").read()
    walk = _definition(fold, "op_fold_slice_row")
    kernels = "".join(_definition(step, name) for name in ("StLine", "st_line", "st_stream_kernel", "st_rows_kernel"))
    d = tmp_path_factory.mktemp("step_host")
    cpp, exe = str(d / "step_host.cpp"), str(d / "step_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(PRELUDE + walk + kernels + MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", exe, cpp], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr) and "error:" not in r.stderr:
        pytest.skip("g++ here has no static AddressSanitizer / UBSan runtime to link")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _hex(a):
    return " ".join(float(x).hex() for x in np.asarray(a).ravel(order="F"))


def _slices(n, p, i, v):
    """The row layout of csrc/otmb_spmv.hip for a matrix without long rows: (val, col, elen, sbase)."""
    A = R.csc_of(n, n, p, i, v).tocsr()  # (CSC -> CSR keeps a row's entries in storage order: the stable transposition)
    lens = np.diff(A.indptr)
    assert lens.max() <= 32  # no row is long
    sbase = [0]
    for s in range((n + 63) // 64):
        sbase.append(sbase[-1] + 64 * int(lens[64 * s:64 * s + 64].max()))
    val, col = np.zeros(sbase[-1]), np.zeros(sbase[-1], dtype=np.int64)
    for r in range(n):
        base = sbase[r >> 6] + (r & 63)
        for e in range(lens[r]):
            val[base + 64 * e], col[base + 64 * e] = A.data[A.indptr[r] + e], A.indices[A.indptr[r] + e]
    return val, col, lens, sbase


def test_rhs_kernels_as_host_code_have_the_bits_of_the_restatement(program):
    exe, path = program
    n, k = N0, 7  # register blocks 4 + 2 + 1; two workgroups, a last slice of one row
    p, i, v = R.dominant(n)
    val, col, elen, sbase = _slices(n, p, i, v)
    rng = np.random.default_rng(1)
    X, S, d = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.uniform(0.0, 1.0, n)
    Xp, Sp = np.full((n + 2, k), np.nan), np.full((n + 3, k), np.nan)  # the padding rows must not be read
    Xp[:n], Sp[:n] = X, S
    W = spmv_ref(n, n, p, i, v, X)
    for theta in (1.0, 0.5, 0.3):
        sigma, c = SR.constants(SR.MONTH, theta)
        for hasd in (0, 1):
            for hass in (0, 1):
                with open(path, "w") as f:
                    f.write(f"{n} {len(val)} {len(sbase) - 1} {k} {hasd} {hass} {float(sigma).hex()} {float(theta).hex()} {float(c).hex()}\n")
                    f.write(f"{_hex(val)}\n{' '.join(map(str, col))}\n{' '.join(map(str, elen))}\n{' '.join(map(str, sbase))}\n")
                    f.write(f"{_hex(d)}\n{_hex(Xp)}\n{_hex(Sp)}\n")
                r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
                assert r.returncode == 0, r.stderr[-3000:]  # (a sanitizer report ends the program with a non-zero status)
                B = np.array([float.fromhex(x) for x in r.stdout.split()]).reshape((n, k), order="F")
                want = SR.rhs(X, None if theta == 1 else W, S if hass else None, d if hasd else None, SR.MONTH, theta)
                assert np.array_equal(B.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (theta, hasd, hass)
