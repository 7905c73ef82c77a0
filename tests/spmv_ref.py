"""Restatement in numpy of SparseArrays' 5-argument mul! for Julia 1.10 (the reference's floor, Project.toml: julia = "1.10"), as
published -- no reference test pins it.  What the device operator (csrc/otmb_spmv.hip, otmb_op_*) must equal bit for bit.

    mul!(Y, A, X, α, β)     LinearAlgebra / SparseArrays, Julia 1.10
      β step first (LinearAlgebra._rmul_or_fill!): β == 0 -> fill!(Y, +0.0) (NaN / Inf already in Y are discarded); β == 1 -> Y as it is;
        otherwise Y[i,c] = Y[i,c] * β.
      A·X (_spmatmul!): for c in 1:k, for col in 1:n: αxj = X[col,c] * α; for j in nzrange(A, col) (stored order):
        Y[rowval[j],c] += nzval[j] * αxj.
        Every Y[i,c] is a left fold that starts from the β step's value (never "the first product": +0.0 + -0.0 is +0.0) and takes its
        contributions in storage order -- by column, inside a column by position; duplicate or unsorted rows are summed in that order.
      Aᵀ·X (_At_or_Ac_mul_B!; real, so the adjoint is the transpose): for c, for col: tmp = +0.0; tmp += nzval[j] * X[rowval[j],c] in
        stored order; Y[col,c] += tmp * α (an empty column adds +0.0 * α).
      No FMA anywhere.  `A * x` and `A' * v` are mul!(…, true, false): α = 1.0, β = 0.0 give the same bits.

np.add.at applies repeated indices one after another in index order (what tests/spmatmul_ref.py relies on too), so each fold below runs in
storage order; every product is formed on its own before it is added (numpy never fuses)."""
import numpy as np


def beta_step(Y, beta):
    Y = np.array(Y, dtype=np.float64, copy=True)
    if beta == 0:
        return np.zeros_like(Y)
    if beta == 1:
        return Y
    return Y * np.float64(beta)


def spmv_ref(m, n, colptr, rowval, nzval, X, alpha=1.0, beta=0.0, Y=None, adjoint=False):
    """α·A·X + β·Y (adjoint: α·Aᵀ·X + β·Y) for the m x n SparseMatrixCSC (colptr, rowval, nzval; 1-based).  X: (rows,) or (rows, k);
    Y: None (β must then be 0) or the result's shape.  Returns a new array of the result's shape."""
    colptr = np.asarray(colptr, dtype=np.int64)
    nnz = int(colptr[-1] - 1)
    rv = np.asarray(rowval, dtype=np.int64)[:nnz] - 1
    nz = np.asarray(nzval, dtype=np.float64)[:nnz]
    X = np.asarray(X, dtype=np.float64)
    vec = X.ndim == 1
    X2 = X.reshape(-1, 1) if vec else X
    k = X2.shape[1]
    ry = n if adjoint else m
    if Y is None:
        assert beta == 0, "beta != 0 needs Y"
        Y = np.zeros((ry, k))
    Y2 = beta_step(np.asarray(Y, dtype=np.float64).reshape(ry, k), beta)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(colptr))  # the column of every stored entry
    a = np.float64(alpha)
    for c in range(k):
        if not adjoint:
            axj = X2[:, c] * a                       # αxj = X[col,c] * α
            prod = nz * axj[col]                     # nzval[j] * αxj
            y = Y2[:, c].copy()
            np.add.at(y, rv, prod)                   # Y[rowval[j],c] += ..., in storage order
            Y2[:, c] = y
        else:
            tmp = np.zeros(n)                        # tmp = +0.0 per column
            np.add.at(tmp, col, nz * X2[rv, c])      # tmp += nzval[j] * X[rowval[j],c], in storage order
            Y2[:, c] = Y2[:, c] + tmp * a            # Y[col,c] += tmp * α
    return Y2.reshape(ry) if vec else Y2


def spmv_loop(m, n, colptr, rowval, nzval, X, alpha=1.0, beta=0.0, Y=None, adjoint=False):
    """The same contract as a literal triple loop over Python floats (the self-test's yardstick)."""
    X = np.asarray(X, dtype=np.float64)
    vec = X.ndim == 1
    X2 = X.reshape(-1, 1) if vec else X
    k = X2.shape[1]
    ry = n if adjoint else m
    if Y is None:
        Y = np.zeros((ry, k))
    Yin = np.asarray(Y, dtype=np.float64).reshape(ry, k)
    out = [[0.0] * k for _ in range(ry)]
    for i in range(ry):
        for c in range(k):
            y = float(Yin[i, c])
            out[i][c] = 0.0 if beta == 0 else (y if beta == 1 else y * float(beta))
    for c in range(k):
        for cl in range(n):
            if not adjoint:
                axj = float(X2[cl, c]) * float(alpha)
                for j in range(int(colptr[cl]) - 1, int(colptr[cl + 1]) - 1):
                    r = int(rowval[j]) - 1
                    out[r][c] = out[r][c] + float(nzval[j]) * axj
            else:
                tmp = 0.0
                for j in range(int(colptr[cl]) - 1, int(colptr[cl + 1]) - 1):
                    tmp = tmp + float(nzval[j]) * float(X2[int(rowval[j]) - 1, c])
                out[cl][c] = out[cl][c] + tmp * float(alpha)
    res = np.array(out, dtype=np.float64).reshape(ry, k)
    return res.reshape(ry) if vec else res


def bits(v):
    """Bit patterns with every NaN the same (a NaN's payload / sign is the hardware's: not part of the contract)."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.int64).copy()
    b[np.isnan(v)] = 0x7FF8000000000000
    return b


def random_csc(rng, m, n, density=0.3, dup=True, unsorted=True, specials=True):
    """A random m x n SparseMatrixCSC (1-based arrays) with empty rows / columns, duplicate and unsorted rows inside a column, stored
    zeros, ±0.0, NaN and Inf."""
    colptr, rowval, nzval = [1], [], []
    for c in range(n):
        cnt = rng.binomial(max(m, 1), density) if m > 0 else 0
        rows = list(rng.choice(m, size=cnt, replace=False) + 1) if cnt else []
        if not unsorted:
            rows.sort()
        if dup and rows and rng.random() < 0.5:
            rows += list(rng.choice(rows, size=int(rng.integers(1, 3))))
        rowval += rows
        colptr.append(colptr[-1] + len(rows))
    vals = rng.standard_normal(len(rowval)) * 10.0 ** rng.integers(-8, 8, len(rowval))
    if specials and len(vals):
        pick = rng.random(len(vals))
        vals[pick < 0.06] = 0.0
        vals[(pick >= 0.06) & (pick < 0.1)] = -0.0
        vals[(pick >= 0.1) & (pick < 0.12)] = np.nan
        vals[(pick >= 0.12) & (pick < 0.14)] = np.inf
        vals[(pick >= 0.14) & (pick < 0.16)] = -np.inf
    return (np.array(colptr, dtype=np.int64), np.array(rowval, dtype=np.int64), vals.astype(np.float64))


def random_dense(rng, rows, k, specials=True):
    X = rng.standard_normal((rows, k)) * 10.0 ** rng.integers(-4, 4, (rows, k))
    if specials and X.size:
        pick = rng.random((rows, k))
        X[pick < 0.05] = 0.0
        X[(pick >= 0.05) & (pick < 0.1)] = -0.0
        X[(pick >= 0.1) & (pick < 0.12)] = np.nan
        X[(pick >= 0.12) & (pick < 0.14)] = np.inf
    return np.asfortranarray(X)
