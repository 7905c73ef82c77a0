"""The device solver's bits on a fixed list of small systems, one JSON line per solve: for comparing two builds of the library.

    python tools/solve_bits.py [--out FILE.jsonl]

Nothing in the suite pins the solver's bits to anything outside itself (its tests bound a residual), so a change that must not alter
them -- a refactor of csrc/otmb_solve.hip or of the operator's layouts -- is checked by running this file in both checkouts on the same
machine: the two outputs must be byte-identical.  It uses api.DeviceOperator only.  Each line: the system, the SHA-256 of X's bytes, the
iterations, the bytes of relres (hex) and the reasons.  The hashes are evidence of one comparison, not expected values: they depend on the
reduction trees and are free to change with them.

Systems (tests/solve_ref.py):
    arrow     arrow(600): row 0 has 600 entries, beyond SP_ELL_MAX = 256 and SP_TCH = 512 -- the long-row kernel with two LDS chunks;
              under the adjoint column 0 is clipped across a chunk edge
    dominant  dominant(257): random, nonsymmetric, about 9 entries per row -- two workgroups of the row kernel, five of the column
              kernel, a last slice of one row
each with A and Aᵀ, with and without d, σ in {0, 0.5} and k in {1, 7, 65} right-hand sides (7 = register blocks of 4 + 2 + 1, 65 = a
second group of 64 columns in the long-row kernel); then, per system and side, one solve with a NaN in one column of B and one with x0."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import otmb_amd.api as api  # noqa: E402
import solve_ref as R  # noqa: E402

RTOL = 1e-10
MAXITER = 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def solve(D, what, B, **kw):
        X, info = D.solve(B, rtol=RTOL, maxiter=MAXITER, **kw)
        rec = dict(what, x_sha256=hashlib.sha256(np.asfortranarray(X).tobytes(order="F")).hexdigest(), iterations=info.iterations.tolist(),
                   relres=info.relres.astype("<f8").tobytes().hex(), reason=list(info.reason))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for name, n, (p, i, v) in (("arrow", 600, R.arrow(600)), ("dominant", 257, R.dominant(257))):
        rng = np.random.default_rng(12)
        d = rng.uniform(0.0, 1.0, n)
        B = np.ones((n, 65), order="F")
        B[:, 1:] = rng.standard_normal((n, 64))
        with api.DeviceOperator(api.SparseMatrixCSC(n, n, p, i, v)) as D:
            for adjoint in (False, True):
                for dd in (None, d):
                    for sigma in (0.0, 0.5):
                        for k in (1, 7, 65):
                            solve(D, dict(system=name, adjoint=adjoint, d=dd is not None, sigma=sigma, k=k), B[:, :k].copy(order="F"), d=dd,
                                  sigma=sigma, adjoint=adjoint)
                Bn = B[:, :7].copy(order="F")
                Bn[n // 2, 3] = np.nan
                solve(D, dict(system=name, adjoint=adjoint, d=True, sigma=0.5, k=7, nan_in_column=3), Bn, d=d, sigma=0.5, adjoint=adjoint)
                solve(D, dict(system=name, adjoint=adjoint, d=True, sigma=0.5, k=7, x0=True), B[:, :7].copy(order="F"), d=d, sigma=0.5, adjoint=adjoint,
                      x0=rng.standard_normal((n, 7)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
