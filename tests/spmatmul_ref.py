"""A numpy restatement of SparseArrays' spmatmul (C = A * B for SparseMatrixCSC{Float64,Int64}) and of the coarse operator
LUMP * T * SPRAY that the reference's workflow forms (src/extratools.jl:14-16, test/local_full.jl:161).  Test infrastructure.

spmatmul, restated from SparseArrays as published: column j of C walks B's stored entries (k, b) of column j in stored order
and, for each, A's stored entries (i, a) of column k in stored order; the first touch of row i COPIES a * b, later touches add
it; rows come out ascending and every touched row is stored, exact zeros included.  `LUMP * T * SPRAY` is the 3-argument `*`,
which LinearAlgebra's _tri_matmul evaluates as (LUMP * T) * SPRAY for these shapes (the two costs are equal).

Vectorised: the contributions are expanded in iteration order, every one finds its (column, row) slot, and np.add.at (which
applies repeated indices in order) sums them into an accumulator initialised to -0.0: -0.0 + x == x bit for bit for every x,
which is the first-touch copy.

Matrices are (m, n, colptr, rowval, nzval) tuples with 1-based colptr / rowval, or objects with those attributes."""
import numpy as np


def _parts(X):
    if isinstance(X, tuple):
        m, n, p, i, v = X
    else:
        m, n, p, i, v = X.m, X.n, X.colptr, X.rowval, X.nzval
    p = np.asarray(p, dtype=np.int64)
    nnz = int(p[-1]) - 1
    return int(m), int(n), p, np.asarray(i, dtype=np.int64)[:nnz], np.asarray(v, dtype=np.float64)[:nnz]


def spmatmul(A, B):
    """C = A * B with spmatmul's semantics -> (m, n, colptr, rowval, nzval), 1-based."""
    m, N, Ap, Ai, Ax = _parts(A)
    NB, n, Bp, Bi, Bx = _parts(B)
    if NB != N:
        raise ValueError(f"DimensionMismatch: A is {m}x{N}, B is {NB}x{n}")
    bcol = np.repeat(np.arange(n, dtype=np.int64), np.diff(Bp))  # column of every entry of B (stored order)
    k = Bi - 1
    cnt = Ap[k + 1] - Ap[k]                                      # A's entries in column k, for every entry of B
    rep = np.repeat(np.arange(len(Bi), dtype=np.int64), cnt)     # the B entry of every contribution, iteration order
    start = np.cumsum(cnt) - cnt
    apos = (Ap[k] - 1)[rep] + (np.arange(len(rep), dtype=np.int64) - start[rep])
    rows = Ai[apos] - 1
    vals = Ax[apos] * Bx[rep]
    slot = bcol[rep] * max(m, 1) + rows
    uniq, inv = np.unique(slot, return_inverse=True)
    acc = np.full(len(uniq), -0.0)
    np.add.at(acc, inv.reshape(-1), vals)
    ccol = uniq // max(m, 1)
    colptr = np.ones(n + 1, dtype=np.int64)
    colptr[1:] += np.cumsum(np.bincount(ccol, minlength=n)[:n])
    return m, n, colptr, uniq % max(m, 1) + 1, acc


def coarse_ref(L, T, S):
    """LUMP * T * SPRAY = (LUMP * T) * SPRAY: P[i,j] complete before P[i,j] * SPRAY[j,J] enters C[i,J]."""
    return spmatmul(spmatmul(L, T), S)


def flat_ref(L, T, S):
    """The same product summed in ONE level: every (j, k) contribution L[i,k] * T[k,j] * S[j,J] added left to right.  Not what
    Julia computes; tests use it to show that the two orders differ."""
    m, N, Lp, Li, Lx = _parts(L)
    _, M, Tp, Ti, Tx = _parts(T)
    _, n, Sp, Si, Sx = _parts(S)
    out = {}
    for J in range(n):
        for s in range(Sp[J] - 1, Sp[J + 1] - 1):
            j = Si[s] - 1
            for t in range(Tp[j] - 1, Tp[j + 1] - 1):
                k = Ti[t] - 1
                for a in range(Lp[k] - 1, Lp[k + 1] - 1):
                    i = Li[a] - 1
                    x = (Lx[a] * Tx[t]) * Sx[s]
                    out[(J, i)] = x if (J, i) not in out else out[(J, i)] + x
    return out
