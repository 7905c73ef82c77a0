"""CPU: the two new elementwise loops -- cb_combine_kernel of csrc/otmb_combine.hip (the fold of otmb_op_combine_slots, with its terms as
arguments and from the table) and pd_precond_kernel of csrc/otmb_periodic.hip (z = v + q / P) -- text as it stands with the pair loads and
stores under them, compiled as plain C++ and executed lane by lane by a stand-alone host program under AddressSanitizer and UBSan, on arrays
of exactly the sizes the library gives them: the results have the bits of the restatement (tests/periodic_pc_ref.py: combine_ref,
precondition), the destination may be a source, no load is misaligned and nothing outside the arrays is touched.  Nothing loaded into python
is sanitised; the pattern is tests/test_periodic_host.py's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import periodic_pc_ref as PC
import periodic_ref as PR
from test_periodic_host import VECTORS
from test_step_host import PRELUDE, _definition, _hex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc")
CB_SPAN = 2048

MAIN = r"""
template <class F> static void launch(i64 blocks, int bs, F f) {
    for (i64 b = 0; b < blocks; ++b)
        for (int t = 0; t < bs; ++t) { blockIdx.x = (unsigned)b; threadIdx.x = (unsigned)t; f(); }
}
static double *exactly(i64 count) {  // count doubles on a 256-byte base (hipMalloc's alignment) and not one more: the sanitizer sees a step too far
    void *p = nullptr;
    if (posix_memalign(&p, 256, (size_t)(count > 0 ? count : 1) * 8)) abort();
    return (double *)p;
}
// in: count, nslots, nt, dst; the nt terms' slots and weights; nslots arrays of count values; then n, P, v (ld), q (ld), ld = n rounded up to even
// out: slot dst after the fold with the terms as arguments (count), after the fold from the table (count); z (n)
int main(int, char **argv) {
    FILE *f = fopen(argv[1], "r");
    long long count, nslots, nt, dst;
    if (fscanf(f, "%lld %lld %lld %lld", &count, &nslots, &nt, &dst) != 4) return 2;
    std::vector<long long> slot((size_t)nt);
    std::vector<double> wt((size_t)nt);
    for (auto &s : slot) if (fscanf(f, "%lld", &s) != 1) return 2;
    for (auto &w : wt) if (fscanf(f, "%la", &w) != 1) return 2;
    std::vector<double *> a((size_t)nslots), b((size_t)nslots);
    for (long long s = 0; s < nslots; ++s) {
        a[(size_t)s] = exactly(count), b[(size_t)s] = exactly(count);
        for (i64 i = 0; i < count; ++i) { if (fscanf(f, "%la", a[(size_t)s] + i) != 1) return 2; b[(size_t)s][i] = a[(size_t)s][i]; }
    }
    const i64 blocks = (count + CB_SPAN - 1) / CB_SPAN;
    if (nt <= CB_ARGS) {
        CbTerms q = {};
        for (long long t = 0; t < nt; ++t) q.src[t] = a[(size_t)slot[(size_t)t]], q.w[t] = wt[(size_t)t];
        launch(blocks, 256, [&] { cb_combine_kernel<false>(q, nullptr, nullptr, (int)nt, count, a[(size_t)dst]); });
    }
    std::vector<const double *> tsrc((size_t)nt);
    for (long long t = 0; t < nt; ++t) tsrc[(size_t)t] = b[(size_t)slot[(size_t)t]];
    launch(blocks, 256, [&] { cb_combine_kernel<true>(CbTerms{}, tsrc.data(), wt.data(), (int)nt, count, b[(size_t)dst]); });
    for (i64 i = 0; i < count; ++i) printf("%a\n", nt <= CB_ARGS ? a[(size_t)dst][i] : b[(size_t)dst][i]);
    for (i64 i = 0; i < count; ++i) printf("%a\n", b[(size_t)dst][i]);
    for (long long s = 0; s < nslots; ++s) {  // the other slots keep their bits
        if (s == dst) continue;
        for (i64 i = 0; i < count; ++i) if (memcmp(a[(size_t)s] + i, b[(size_t)s] + i, 8)) return 3;
    }
    long long n;
    double P;
    if (fscanf(f, "%lld %la", &n, &P) != 2) return 2;
    const i64 ld = (n + 1) & ~(i64)1;
    double *v = exactly(ld), *qv = exactly(ld), *z = exactly(ld);
    for (i64 i = 0; i < ld; ++i) if (fscanf(f, "%la", v + i) != 1) return 2;
    for (i64 i = 0; i < ld; ++i) if (fscanf(f, "%la", qv + i) != 1) return 2;
    for (i64 i = 0; i < ld; ++i) z[i] = NAN;
    launch((n + PD_ROWS - 1) / PD_ROWS, 256, [&] { pd_precond_kernel(n, v, qv, P, z); });
    for (i64 i = 0; i < n; ++i) printf("%a\n", z[i]);
    if (ld > n && z[n] == z[n]) return 4;  // the padding row was written
    for (long long s = 0; s < nslots; ++s) free(a[(size_t)s]), free(b[(size_t)s]);
    free(v), free(qv), free(z);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this host")
    cb = open(os.path.join(CSRC, "otmb_combine.hip"), encoding="utf-8").read()
    pd = open(os.path.join(CSRC, "otmb_periodic.hip"), encoding="utf-8").read()
    defines = "".join(re.search(r"^#define " + name + r" \d+", text, re.M).group(0) + "\n"
                      for name, text in (("CB_SPAN", cb), ("CB_ARGS", cb), ("PD_ROWS", pd)))
    assert f"#define CB_SPAN {CB_SPAN}\n" in defines and f"#define PD_ROWS {PR.PD_ROWS}\n" in defines
    code = "".join(_definition(cb, name) for name in ("CbTerms", "Cb2", "cb_load", "cb_store", "cb_combine_kernel"))
    code += "".join(_definition(pd, name) for name in ("Pd2", "pd_load", "pd_store", "pd_row", "pd_precond_kernel"))
    d = tmp_path_factory.mktemp("periodic_pc_host")
    cpp, exe = str(d / "periodic_pc_host.cpp"), str(d / "periodic_pc_host")
    with open(cpp, "w", encoding="utf-8") as f:
        f.write(PRELUDE + "#include <cstring>\n" + VECTORS + defines + code + MAIN)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-o", exe, cpp], capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr) and "error:" not in r.stderr:
        pytest.skip("g++ here has no static AddressSanitizer / UBSan runtime to link")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, str(d / "in.txt")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("count,n,w,dst", [
    (1, 1, (0.25, 0.0, 0.75), 0),                                   # one entry, no pair
    (513, 513, (1 / 3, 1 / 3, 1 / 3), 3),                           # lane 0's second pair, of a single entry
    (CB_SPAN, 2048, (0.25, 0.0, 0.75), 3),                          # a workgroup exactly full
    (CB_SPAN + 1, 2049, (0.25, 0.0, 0.75), 0),                      # a second workgroup of one entry (odd: no 16-byte access to it), into a source
    (CB_SPAN + 2, 4609, (1 / 3, 1 / 3, 1 / 3), 2),                  # a second workgroup of one pair, into a source
    (2 * CB_SPAN + 513, 118, (0.0, 0.0, 0.0), 1),                   # no term at all: +0.0
    (1001, 512, tuple(np.random.default_rng(4).uniform(-1, 1, 17)), 16),  # seventeen terms: the table only
])
def test_the_fold_and_the_preconditioned_direction_as_host_code(program, count, n, w, dst):
    exe, path = program
    rng = np.random.default_rng(count + n)
    w = np.array(tuple(w) + ((0.0,) if len(w) == 3 else ()))  # (three weights: a fourth slot that is only written or left alone)
    nslots = len(w)
    values = [rng.standard_normal(count) * 10.0 ** rng.uniform(-6, 6, count) for _ in range(nslots)]
    terms = [s for s in range(nslots) if w[s] != 0.0]
    ld = (n + 1) & ~1
    P = 3 * 2592000.0
    v, q = np.full(ld, np.nan), np.full(ld, np.nan)  # the padding row must be neither read into a result nor written
    v[:n], q[:n] = rng.standard_normal(n), rng.standard_normal(n) * 1e7
    with open(path, "w") as f:
        f.write(f"{count} {nslots} {len(terms)} {dst}\n{' '.join(str(s) for s in terms)}\n{_hex(w[terms])}\n")
        f.write("\n".join(_hex(x) for x in values) + f"\n{n} {float(P).hex()}\n{_hex(v)}\n{_hex(q)}\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])  # (a sanitizer report ends the program with a non-zero status)
    out = np.array([float.fromhex(x) for x in r.stdout.split()])
    assert len(out) == 2 * count + n
    want = PC.combine_ref(values, w)
    assert np.array_equal(_bits(out[:count]), _bits(want)), (count, "the terms as arguments")
    assert np.array_equal(_bits(out[count:2 * count]), _bits(want)), (count, "the terms from the table")
    if not terms:
        assert not np.signbit(out[:2 * count]).any()
    assert np.array_equal(_bits(out[2 * count:]), _bits(PC.precondition(v[:n], q[:n], P))), (n, "z = v + q / P")
