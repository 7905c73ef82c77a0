"""A numpy restatement of the two contracts of include/otmb.h that no function of the reference pins: buildTsink (otmb_build_sink,
csrc/otmb_sink.hip), the settling operator S of particles that sink at a speed w >= 0, and add_matrix (otmb_op_add_matrix,
csrc/otmb_addmat.hip), slot = slot + α·B by positions.  Elementwise float64 numpy is IEEE arithmetic without FMA, so these are the
contracts' bits.

buildTsink, per wet cell c at (i, j, k), ascending in wet order (Julia's column-major order of the wet cells), a = area2D[i, j], w_c the
speed at the bottom face of c, b the wet cell at (i, j, k + 1) if there is one:
    (c, c) = (w_c * a) / v3D[c];    (b, c) = -((w_c * a) / v3D[b]);    seafloor = "closed" and no b: (c, c) = +0.0, stored.
CSC, rows ascending (b > c), every diagonal stored: nnz = N + the wet cells with a wet cell below, whatever w and the seafloor are.

add_matrix: the stored entry (r, c) of B belongs to the FIRST stored entry (r, c) of the operator's column c in stored order; then, for every
requested slot, in B's stored order, nz[p] = nz[p] + (α * B[e]).  Never scipy's `+`, which re-sorts and merges."""
import numpy as np

SEAFLOORS = ("open", "closed")


class BadSpeed(ValueError):
    """w is negative, NaN or infinite on the bottom face of a wet cell (the library: INVALID_ARG)."""


class SinkNaN(ValueError):
    """The result holds a NaN (the library: TSINK_NAN, "Tsink contains NaNs.")."""


class PatternNotContained(ValueError):
    """entry: the 0-based position in B's stored order of the first entry the operator does not store; row, col: 1-based."""

    def __init__(self, entry, row, col):
        super().__init__(f"entry {entry + 1} of B, (row {row}, column {col}), is not stored in the operator")
        self.entry, self.row, self.col = entry, row, col


def wet_indices(v3D):
    """makeindices(v3D) restated: (wet (nx, ny, nz) bool, Lwet3D (wet rank, 1-based, 0 on land), N)."""
    wet = ~np.isnan(np.asarray(v3D, dtype=np.float64))
    flat = wet.ravel(order="F")
    rank = np.where(flat, np.cumsum(flat), 0).astype(np.int64)
    return wet, rank.reshape(wet.shape, order="F"), int(flat.sum())


def speeds(w, shape):
    """w in its three forms as an (nx, ny, nz) array: a scalar, nz values (the bottom face of each level), or the array itself."""
    nx, ny, nz = shape
    w = np.asarray(w, dtype=np.float64)
    if w.ndim == 0:
        return np.full(shape, float(w))
    if w.shape == (nz,):
        return np.broadcast_to(w[None, None, :], shape)
    if w.shape == tuple(shape):
        return w
    raise ValueError(f"w of {w.shape}")


def sink_ref(w, v3D, area2D, seafloor="open"):
    """-> (colptr, rowval, nzval) of S, Julia's arrays (1-based)."""
    assert seafloor in SEAFLOORS
    v3D = np.asarray(v3D, dtype=np.float64)
    nx, ny, nz = v3D.shape
    wet, L3, N = wet_indices(v3D)
    W = speeds(w, v3D.shape)
    lin = np.flatnonzero(wet.ravel(order="F"))  # ascending linear indices of the wet cells: wet order
    i, j, k = np.unravel_index(lin, v3D.shape, order="F")
    wc = W[i, j, k]  # (read on wet cells only)
    if not np.all((wc >= 0.0) & np.isfinite(wc)):
        raise BadSpeed("w must be finite and >= 0 on the bottom face of every wet cell")
    kb = np.minimum(k + 1, nz - 1)
    below = (k + 1 < nz) & wet[i, j, kb]
    b = np.where(below, L3[i, j, kb], 0)  # 1-based wet rank of the cell below
    with np.errstate(all="ignore"):
        wa = wc * np.asarray(area2D, dtype=np.float64)[i, j]
        diag = wa / v3D[i, j, k]
        if seafloor == "closed":
            diag = np.where(below, diag, 0.0)
        off = -(wa / np.where(below, v3D[i, j, kb], 1.0))
    if np.isnan(diag).any() or np.isnan(off[below]).any():
        raise SinkNaN("Tsink contains NaNs.")
    count = 1 + below.astype(np.int64)
    colptr = np.concatenate(([1], 1 + np.cumsum(count))).astype(np.int64)
    nnz = int(colptr[-1] - 1)
    rowval, nzval = np.zeros(nnz, dtype=np.int64), np.zeros(nnz)
    p = colptr[:-1] - 1
    rowval[p], nzval[p] = np.arange(1, N + 1), diag
    rowval[p[below] + 1], nzval[p[below] + 1] = b[below], off[below]
    return colptr, rowval, nzval


def seafloor_flux(w, v3D, area2D, x):
    """Σ over the wet cells without a wet cell below of (w_c * a)·x_c: what leaves through the seafloor faces with seafloor="open"."""
    v3D = np.asarray(v3D, dtype=np.float64)
    nz = v3D.shape[2]
    wet, L3, N = wet_indices(v3D)
    i, j, k = np.unravel_index(np.flatnonzero(wet.ravel(order="F")), v3D.shape, order="F")
    kb = np.minimum(k + 1, nz - 1)
    floor = ~((k + 1 < nz) & wet[i, j, kb])
    wa = speeds(w, v3D.shape)[i, j, k] * np.asarray(area2D, dtype=np.float64)[i, j]
    return float(np.sum(wa[floor] * np.asarray(x)[floor]))


def column_solve(colptr, rowval, nzval, r, s):
    """x with (r·I + S)·x = s by the closed-form downward recursion: S is lower bidiagonal along the water columns (wet order puts the cell
    below behind the cell), so x_c = (s_c - Σ_{c' above} S[c, c']·x_c') / (r + S[c, c]) in ascending c."""
    n = len(colptr) - 1
    x, rhs = np.zeros(n), np.array(s, dtype=np.float64)
    for c in range(n):
        p0, p1 = colptr[c] - 1, colptr[c + 1] - 1
        assert rowval[p0] == c + 1
        x[c] = rhs[c] / (r + nzval[p0])
        for p in range(p0 + 1, p1):
            rhs[rowval[p] - 1] -= nzval[p] * x[c]
    return x


def match_positions(colptr, rowval, Bp, Bi):
    """pos[e]: the position in the operator's stored order of B's stored entry e -- the FIRST stored entry of the operator's column with its
    row.  Raises PatternNotContained for the first entry of B without one."""
    n = len(colptr) - 1
    assert len(Bp) == n + 1
    pos = np.zeros(int(Bp[-1]) - 1, dtype=np.int64)
    for c in range(n):
        rows = rowval[colptr[c] - 1 : colptr[c + 1] - 1]
        for e in range(Bp[c] - 1, Bp[c + 1] - 1):
            hit = np.flatnonzero(rows == Bi[e])
            if not hit.size:
                raise PatternNotContained(e, int(Bi[e]), c + 1)
            pos[e] = colptr[c] - 1 + hit[0]
    return pos


def add_matrix_ref(colptr, rowval, values, B, alpha=1.0, slots=None):
    """values: the slots' nzval arrays.  -> the new list: slot s in `slots` (None: all) has nz[p] = nz[p] + (alpha * B[e]) for B's entries in
    stored order, the others are the arrays given.  alpha == 0 matches (and may raise) and writes nothing."""
    Bp, Bi, Bx = B
    pos = match_positions(np.asarray(colptr), np.asarray(rowval), np.asarray(Bp), np.asarray(Bi))
    sel = range(len(values)) if slots is None else [int(s) for s in np.atleast_1d(slots)]
    out = [np.array(v, dtype=np.float64) for v in values]
    if alpha == 0.0:
        return out
    t = np.float64(alpha) * np.asarray(Bx, dtype=np.float64)[: len(pos)]
    for s in sel:
        for e, p in enumerate(pos):  # (one addition per stored entry of B, in B's order: a position named twice is added to twice)
            out[s][p] = out[s][p] + t[e]
    return out


# ---- the hand-made grids of the tests -----------------------------------------------------------------------------------------------
GAP_WET = {  # (i, j) -> the wet levels of a 3 x 2 x 5 grid: a dry cell inside two columns, a column of one cell, a dry column
    (0, 0): (0, 1, 2, 3, 4),
    (1, 0): (0, 1, 3, 4),  # level 2 is dry: the flux is cut there
    (2, 0): (0, 1, 2),
    (0, 1): (0,),
    (1, 1): (),
    (2, 1): (0, 2, 3),  # level 1 is dry
}


def gap_grid(seed=4):
    """(v3D, area2D) of the gap mask: random positive volumes and areas, NaN on the dry cells."""
    rng = np.random.default_rng(seed)
    v3D = np.full((3, 2, 5), np.nan, order="F")
    for (i, j), levels in GAP_WET.items():
        for k in levels:
            v3D[i, j, k] = rng.uniform(1e12, 5e13)
    return v3D, np.asfortranarray(rng.uniform(1e10, 9e10, (3, 2)))


def one_level_grid(seed=6):
    """(v3D, area2D) of a 9 x 7 x 1 grid with some land: no vertical pair at all."""
    rng = np.random.default_rng(seed)
    v3D = np.asfortranarray(rng.uniform(1e12, 5e13, (9, 7, 1)))
    v3D[rng.random((9, 7, 1)) < 0.3] = np.nan
    return v3D, np.asfortranarray(rng.uniform(1e10, 9e10, (9, 7)))
