"""CPU: the device code of the line preconditioner (the kernels of csrc/otmb_solve_lines.hip, text as it stands) compiled as plain C++ and
executed lane by lane by a stand-alone host program, under AddressSanitizer and UBSan, on arrays of exactly the sizes the library
allocates: the validation, the heads table, the extraction, the factorisation and the sweep have the bits of the numpy restatement
(tests/solve_lines_ref.py) and touch nothing outside their arrays.  It says nothing about concurrency; no two lanes of these kernels write
the same element (a line has one owner), which is what makes a sequential run a fair stand-in for the arithmetic and the index work."""
import os
import subprocess

import numpy as np
import pytest

import solve_lines_ref as LR
import solve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc", "otmb_solve_lines.hip")
N0 = 257

PRELUDE = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
typedef int64_t i64;
#define __global__
#define __restrict__
#define __launch_bounds__(x)
struct Dim { unsigned x; };
static Dim blockIdx, threadIdx;
template <class T> static void atomicMin(T *p, T v) { if (v < *p) *p = v; }
static void atomicAdd(int *p, int v) { *p += v; }
using std::isfinite;
enum { SV_ACTIVE = 0 };
struct SvCol { double rho, alpha, omega, beta, bnorm, relres, rhn; int state, reason, restart, bzero; i64 iters; };
"""

MAIN = r"""
template <class F> static void launch(i64 blocks, int bs, F f) {
    for (i64 b = 0; b < blocks; ++b)
        for (int t = 0; t < bs; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t; f(); }
}
// in: n, next[n], nnz, colptr[n+1] (1-based), rows[nnz] (0-based), nzval[nnz], diag[n], adjoint, k, Y[n*k]; out: a verdict, then Z
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long n, nnz, x;
    int adjoint, k;
    if (fscanf(f, "%lld", &n) != 1) return 2;
    std::vector<i64> next(n), cp(n + 1);
    for (auto &v : next) { if (fscanf(f, "%lld", &x) != 1) return 2; v = x; }
    if (fscanf(f, "%lld", &nnz) != 1) return 2;
    for (auto &v : cp) { if (fscanf(f, "%lld", &x) != 1) return 2; v = x; }
    std::vector<int> rv(nnz);
    std::vector<double> nz(nnz), diag(n);
    for (auto &v : rv) if (fscanf(f, "%d", &v) != 1) return 2;
    for (auto &v : nz) if (fscanf(f, "%la", &v) != 1) return 2;
    for (auto &v : diag) if (fscanf(f, "%la", &v) != 1) return 2;
    if (fscanf(f, "%d %d", &adjoint, &k) != 2) return 2;
    std::vector<double> Y((size_t)n * k);
    for (auto &v : Y) if (fscanf(f, "%la", &v) != 1) return 2;
    std::vector<int> nxt(n), prv(n, -1), cnt(n, 0);
    std::vector<i64> flag(n + 1), pos(n + 1);
    ull bad[2] = {~0ull, ~0ull};
    launch((n + 255) / 256, 256, [&] { ln_check_kernel(next.data(), n, nxt.data(), prv.data(), cnt.data(), bad); });
    launch((n + 256) / 256, 256, [&] { ln_flag_kernel(cnt.data(), n, flag.data(), bad + 1); });
    if (bad[0] != ~0ull) { printf("range %llu\n", bad[0]); return 0; }
    if (bad[1] != ~0ull) { printf("twice %llu\n", bad[1]); return 0; }
    i64 acc = 0;
    for (i64 i = 0; i <= n; ++i) { pos[i] = acc; acc += flag[i]; }  // (the library: rocprim's exclusive scan)
    const i64 nheads = pos[n];
    std::vector<int> heads(nheads);
    launch((n + 255) / 256, 256, [&] { ln_heads_kernel(flag.data(), pos.data(), n, heads.data()); });
    std::vector<double> u(n), m(n), piv(n);
    launch((n + 255) / 256, 256, [&] { ln_ul_kernel(cp.data(), rv.data(), nz.data(), n, nxt.data(), adjoint, u.data(), m.data()); });
    ull pb = ~0ull;
    launch((nheads + 63) / 64, 64, [&] { ln_factor_kernel(heads.data(), nheads, nxt.data(), diag.data(), u.data(), m.data(), piv.data(), &pb); });
    if (pb != ~0ull) { printf("pivot %llu\n", pb); return 0; }
    std::vector<double> Z((size_t)n * k, 7.25);
    int c0 = 0;
    for (int kb : {4, 2, 1})  // op_blocks<SV_KB>
        for (; k - c0 >= kb; c0 += kb) {
            const double *y = Y.data() + (size_t)c0 * n;
            double *z = Z.data() + (size_t)c0 * n;
            launch((nheads + 63) / 64, 64, [&] {
                if (kb == 4) ln_sweep_kernel<4>(nullptr, heads.data(), nheads, nxt.data(), prv.data(), m.data(), u.data(), piv.data(), y, n, z, n);
                if (kb == 2) ln_sweep_kernel<2>(nullptr, heads.data(), nheads, nxt.data(), prv.data(), m.data(), u.data(), piv.data(), y, n, z, n);
                if (kb == 1) ln_sweep_kernel<1>(nullptr, heads.data(), nheads, nxt.data(), prv.data(), m.data(), u.data(), piv.data(), y, n, z, n);
            });
        }
    printf("ok %lld\n", (long long)nheads);
    for (double v : Z) printf("%a\n", v);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    src = open(SRC, encoding="utf-8").read()
    kernels = src[src.index("typedef unsigned long long ull;"):src.index("// ---- host")]
    assert "__global__" in kernels and "ln_sweep_kernel" in kernels
    d = tmp_path_factory.mktemp("lines_host")
    cpp, exe = str(d / "lines_host.cpp"), str(d / "lines_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(PRELUDE + kernels + MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", exe, cpp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _hex(a):
    return " ".join(float(x).hex() for x in np.asarray(a).ravel(order="F"))


def _run(program, A, nxt, diag, adjoint, Y):
    exe, path = program
    n, k = Y.shape
    A = A.tocsc()
    with open(path, "w") as f:
        f.write(f"{n}\n{' '.join(map(str, nxt))}\n{A.nnz}\n{' '.join(map(str, A.indptr + 1))}\n{' '.join(map(str, A.indices))}\n")
        f.write(f"{_hex(A.data)}\n{_hex(diag)}\n{int(adjoint)} {k}\n{_hex(Y)}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]  # (a sanitizer report ends the program with a non-zero status)
    out = r.stdout.split("\n")
    Z = np.array([float.fromhex(x) for x in out[1:] if x]).reshape((n, k), order="F") if out[0].startswith("ok") else None
    return out[0], Z


LINE_SETS = [np.zeros(N0, dtype=np.int64), LR.stride_lines(N0, 1), LR.stride_lines(N0, 64), LR.stride_lines(N0, 65)] + \
            [LR.random_lines(N0, s) for s in range(6)]


def test_kernels_as_host_code_have_the_bits_of_the_restatement(program):
    p, i, v = R.dominant(N0)
    A = R.csc_of(N0, N0, p, i, v)
    d = np.random.default_rng(13).uniform(0.0, 1.0, N0)
    diag = R.jacobi_diagonal(A, d, 0.5)
    Y = np.asfortranarray(np.random.default_rng(3).standard_normal((N0, 7)))
    for nxt in LINE_SETS:
        for adjoint in (False, True):
            P = LR.Lines(A, nxt, d, 0.5, adjoint)
            want = P.apply(Y)
            for k in (1, 7):  # register blocks 1; 4 + 2 + 1
                verdict, Z = _run(program, A, nxt, diag, adjoint, Y[:, :k])
                assert verdict == f"ok {len(P.heads)}"
                assert np.array_equal(Z.view(np.uint64), want[:, :k].view(np.uint64)), (adjoint, k)


def test_kernels_as_host_code_refuse_what_the_restatement_refuses(program):
    import scipy.sparse as sp

    A = R.csc_of(N0, N0, *R.dominant(N0))
    diag = R.jacobi_diagonal(A)
    Y = np.ones((N0, 1), order="F")
    for at, val in ((100, 101), (100, 7), (100, N0 + 1), (100, -3), (N0 - 1, N0)):
        bad = np.zeros(N0, dtype=np.int64)
        bad[at], bad[200] = val, 1
        assert _run(program, A, bad, diag, False, Y)[0] == f"range {min(at, 200)}"
    bad = np.zeros(N0, dtype=np.int64)
    bad[[3, 5, 10, 11]] = (50, 50, 40, 40)
    assert _run(program, A, bad, diag, False, Y)[0] == "twice 39"
    Z = sp.csc_matrix(np.array([[2.0, 4.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))
    assert _run(program, Z, np.array([2, 0, 0]), R.jacobi_diagonal(Z), False, np.ones((3, 1), order="F"))[0] == "pivot 1"
