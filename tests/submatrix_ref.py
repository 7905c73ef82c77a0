"""A numpy restatement of otmb_op_submatrix's rule (include/otmb.h, csrc/otmb_submatrix.hip): for ascending selections `rows` and `cols`
(0-based here), column j' of the child holds the stored entries of column cols[j'] whose row is selected, in stored order, rows renumbered
by their rank in `rows`; src[p] is the position of the child's entry p in the parent's nzval (the gather table); and the lines of a
principal selection: next'[rank(i)] = rank(next[i]) where i and next[i] are both selected, 0 elsewhere.  It states the rule and nothing of
how the device does it: no scan, no scatter."""
import numpy as np


def first_offender(idx, limit):
    """The refusal rule: the first 0-based position of a 1-based index list whose entry is outside 1..limit or not above the entry before
    it; None when the list ascends strictly inside 1..limit."""
    idx = np.asarray(idx, dtype=np.int64)
    bad = (idx < 1) | (idx > limit)
    bad[1:] |= idx[1:] <= idx[:-1]
    hit = np.flatnonzero(bad)
    return int(hit[0]) if hit.size else None


def ranks(sel, limit):
    """rank[i] = the position of i in the ascending 0-based selection, -1 when dropped."""
    sel = np.asarray(sel, dtype=np.int64)
    assert first_offender(sel + 1, limit) is None
    r = np.full(limit, -1, dtype=np.int64)
    r[sel] = np.arange(len(sel))
    return r


def submatrix_ref(m, n, colptr, rowval, rows, cols):
    """-> (colptr', rowval', src): the child's 1-based colptr (len(cols) + 1) and rowval, and src (0-based positions in the parent's nzval)."""
    cp = np.asarray(colptr, dtype=np.int64)
    nnz = int(cp[-1] - 1)
    rv = np.asarray(rowval, dtype=np.int64)[:nnz] - 1
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(cp))
    rrank, crank = ranks(rows, m), ranks(cols, n)
    src = np.flatnonzero((rrank[rv] >= 0) & (crank[col] >= 0))  # ascending positions: by column, inside a column in stored order
    counts = np.bincount(crank[col[src]], minlength=len(cols)).astype(np.int64)
    cpc = np.concatenate([[1], 1 + np.cumsum(counts)]).astype(np.int64)
    return cpc, rrank[rv[src]] + 1, src


def submatrix_values(nzval, src):
    return np.asarray(nzval, dtype=np.float64)[src]


def restrict_lines(next, sel):
    """next (1-based successors, 0 = none) of n unknowns restricted to the ascending 0-based selection `sel`."""
    nx = np.asarray(next, dtype=np.int64)
    sel = np.asarray(sel, dtype=np.int64)
    rank = ranks(sel, len(nx))
    succ = nx[sel] - 1  # -1: none
    out = np.zeros(len(sel), dtype=np.int64)
    has = succ >= 0
    out[has] = rank[succ[has]] + 1  # a dropped successor has rank -1: 0
    return out
