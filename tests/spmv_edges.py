"""Fixtures at the layout thresholds of the resident sparse operator (csrc/otmb_spmv.hip, otmb_op_*), and a mirror of its layout rule.

The mirror (layout, tracer_blocks, tracer_groups) restates the rule as the kernel file's header and plan state it: rows in slices of 64
(the last one may be partial); a row is long if len > SP_ELL_MAX (256), or if len > 32 and len > 4·mean, mean = ceil(sum of the slice's
row lengths / rows in the slice); long rows are folded in chunks of SP_TCH (512) entries, tracers in groups of 64; Aᵀ·X takes 64 columns
per wave and stages the wave's run of entries in chunks of 512; tracers go in register blocks of 8, 4, 2 and 1.  It is used only to show
that a fixture lands on the side of a threshold it claims.  It never gives an expected result: tests/spmv_ref.py is the only reference.

A fixture is a named m x n SparseMatrixCSC (1-based colptr, rowval, nzval) and `focus`: for each path it is meant to reach ("rows":
spmv_rows_kernel, "long": spmv_long_kernel, "cols": spmv_cols_kernel), the 0-based output elements it is about (rows of A·X, columns of
A for Aᵀ·X).  Entries lie in random order inside a column (unsorted rows) and a row may be drawn twice for one column (duplicates).
Values spread over 16 decades, as random_csc's do, with stored ±0.0; NaN and ±Inf sit in entries marked dirty, which no focus element
reads (the size fixtures are random_csc's own, specials anywhere).  Values are drawn again until each focus path has an element whose
storage-order fold differs from the reversed one."""
import functools
from types import SimpleNamespace

import numpy as np

from spmv_ref import bits, random_csc, spmv_ref

SLICE = 64       # rows per slice (one wave of spmv_rows_kernel)
ELL_MAX = 256    # SP_ELL_MAX
TCH = 512        # SP_TCH: entries per LDS chunk (long rows, Aᵀ runs)
WAVE = 64        # columns per wave of spmv_cols_kernel
ROWS_WG = 256    # rows per workgroup of spmv_rows_kernel
GROUP = 64       # tracers per pass of spmv_long_kernel
PLAN_THREADS = 65536 * 256  # SP_GRID's cap: the plan kernels loop beyond it

K_BASE = (1, 3, 8)
K_LONG = (63, 64, 65, 128, 129)        # on fixtures with a long row
K_SPLITS = tuple(range(1, 18)) + (24,)  # every 8/4/2/1 split
BIG = (1 << 24) + 197                   # m = n of the matrix above 2^24 (197 = 3·64 + 5: a partial last slice)


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def layout(m, n, colptr, rowval):
    """The layout the plan builds, as counts: per row its length and whether it is long; per slice its rows, mean and width; per Aᵀ wave
    its run of entries; per column the chunk edges it crosses (as the number of its entries before each edge)."""
    cp = np.asarray(colptr, dtype=np.int64)
    nnz = int(cp[-1] - 1)
    lens = np.bincount(np.asarray(rowval, dtype=np.int64)[:nnz] - 1, minlength=m).astype(np.int64)
    ns = -(-m // SLICE)
    L = np.zeros(ns * SLICE, dtype=np.int64)
    L[:m] = lens
    L = L.reshape(ns, SLICE)
    rows = np.minimum(SLICE, m - SLICE * np.arange(ns))
    mean = -(-L.sum(axis=1) // np.maximum(rows, 1))
    lng = (L > ELL_MAX) | ((L > 32) & (L > 4 * mean[:, None]))
    width = np.where(lng, 0, L).max(axis=1) if ns else np.zeros(0, dtype=np.int64)
    nw = -(-n // WAVE)
    first = WAVE * np.arange(nw)
    wb = cp[first]
    run = cp[np.minimum(first + WAVE, n)] - wb
    c = np.arange(n)
    a, b = cp[c] - wb[c // WAVE], cp[c + 1] - wb[c // WAVE]  # a column's entries relative to its wave's run
    cross = {}
    for j in np.flatnonzero((a // TCH + 1) * TCH < b):  # some edge e = 512 t with a < e < b
        cross[int(j)] = [int(e - a[j]) for e in range((a[j] // TCH + 1) * TCH, b[j], TCH)]
    return SimpleNamespace(lens=lens, long=lng.reshape(-1)[:m], nslices=ns, slice_rows=rows, mean=mean, width=width, waves=nw, run=run,
                           cross=cross, row_wgs=-(-m // ROWS_WG))


def long_chunks(length):
    return -(-length // TCH)


def tracer_blocks(k):
    """The register blocks otmb_op_mul_dev launches for k tracers, in order."""
    out = []
    while k > 0:
        b = next(b for b in (8, 4, 2, 1) if k >= b)
        out.append(b)
        k -= b
    return out


def tracer_groups(k):
    return -(-k // GROUP)


# ---- builders -----------------------------------------------------------------------------------------------------------------------
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan, np.inf, -np.inf)


def _pattern(rng, n, rows, cols, dirty=None):
    """(colptr, rowval, draw) of the entries (rows[e], cols[e]) (0-based): sorted by column, in random order inside a column (1-based).
    draw(rng) gives values of widely spread magnitude with about 10 % stored ±0.0, and SPECIALS at entries where `dirty` holds."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.lexsort((rng.random(len(rows)), cols))
    rows, cols = rows[order], cols[order]
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    nnz = len(rows)
    d = None if dirty is None else np.flatnonzero(np.asarray(dirty)[order])

    def draw(rng):
        v = rng.standard_normal(nnz) * 10.0 ** rng.integers(-8, 8, nnz)
        pick = rng.random(nnz)
        v[pick < 0.06] = 0.0
        v[(pick >= 0.06) & (pick < 0.1)] = -0.0
        if d is not None:
            sel = np.sort(rng.choice(d, size=min(len(d), len(SPECIALS)), replace=False))
            v[sel] = SPECIALS[:len(sel)]
        return v

    return colptr, rows + 1, draw


def _rows_entries(rng, n, lens):
    """Row i gets lens[i] entries, in columns drawn with replacement (a column can hold row i twice)."""
    rows = np.repeat(np.arange(len(lens)), lens)
    return rows, rng.integers(0, n, len(rows))


def _cols_entries(rng, m, lens):
    cols = np.repeat(np.arange(len(lens)), lens)
    return rng.integers(0, m, len(cols)), cols


class Fixture(SimpleNamespace):
    """name, m, n, colptr, rowval, nzval; focus: {path: 0-based output elements}."""

    @property
    def A(self):
        return (self.m, self.n, self.colptr, self.rowval, self.nzval)


def _fx(name, m, n, rng, make, focus):
    """The first draw of make(rng) -> (colptr, rowval, nzval) whose every focus path tells a reversed fold from the storage-order one."""
    for _ in range(100):
        p, i, v = make(rng)
        f = Fixture(name=name, m=m, n=n, colptr=p, rowval=i, nzval=v, focus={k: np.asarray(e, dtype=np.int64) for k, e in focus.items()})
        if all(order_sensitive(f, path) for path in f.focus):
            return f
    raise AssertionError(f"{name}: no draw of values is order sensitive on every focus path")


def _values(pattern):
    p, i, draw = pattern
    return lambda rng: (p, i, draw(rng))


def _absolute(name, L, seed):
    """64 rows: 63 of 61 entries and row 17 of L (256: short, 257: long).  mean = ceil((3843 + L) / 64) = 65, 4·mean = 260 >= L: only the
    absolute rule (L > 256) decides."""
    rng = np.random.default_rng(seed)
    m, n, t = 64, 300, 17
    lens = np.full(m, 61)
    lens[t] = L
    r, c = _rows_entries(rng, n, lens)
    focus = {"long": [t], "rows": np.delete(np.arange(m), t)} if L > ELL_MAX else {"rows": [t]}
    return _fx(name, m, n, rng, _values(_pattern(rng, n, r, c)), {**focus, "cols": np.arange(n)})


def _relative(name, m, t, L, others, seed):
    """Row t of length L in a slice whose other rows hold `others` (a list of lengths, each <= 32); rows of other slices: 3-6 entries."""
    rng = np.random.default_rng(seed)
    n = 300
    lens = rng.integers(3, 7, m)
    s0 = (t // SLICE) * SLICE
    idx = [i for i in range(s0, min(s0 + SLICE, m)) if i != t]
    lens[idx] = others
    lens[t] = L
    r, c = _rows_entries(rng, n, lens)
    pat = _pattern(rng, n, r, c)
    lng = layout(m, n, *pat[:2]).long
    focus = {"long": [t], "rows": np.flatnonzero(~lng)} if lng[t] else {"rows": [t]}
    return _fx(name, m, n, rng, _values(pat), {**focus, "cols": np.arange(n)})


def _long_rows(name, L, seed):
    """130 rows (the last slice holds two): row 10 and row 129 have L entries (long by the absolute rule), the others 2-6.  Row 129 carries
    NaN, ±Inf and ±0.0; row 10 (the focus) does not."""
    rng = np.random.default_rng(seed)
    m, n = 130, 300
    lens = rng.integers(2, 7, m)
    lens[[10, 129]] = L
    r, c = _rows_entries(rng, n, lens)
    short = np.flatnonzero(lens <= 6)
    return _fx(name, m, n, rng, _values(_pattern(rng, n, r, c, dirty=(r == 129))), {"long": [10], "rows": short, "cols": np.arange(n)})


def _run(name, total, seed):
    """One Aᵀ wave (64 columns) whose run holds `total` entries: column 0 has 200, columns 1-62 four each, column 63 the rest (64 or 65:
    with 65 it crosses the chunk edge after 63 of them)."""
    rng = np.random.default_rng(seed)
    m, n = 300, 64
    lens = np.full(n, 4)
    lens[0] = 200
    lens[63] = total - 200 - 4 * 62
    r, c = _cols_entries(rng, m, lens)
    return _fx(name, m, n, rng, _values(_pattern(rng, n, r, c)), {"cols": [0, 63], "rows": np.arange(m)})


STRADDLE = ((1, 511, 3), (3, 256, 100), (17, 63, 40), (40, 2, 7), (63, 1, 1), (0, 512, 588))  # (column in its wave, entries before the edge, after)
STRADDLE_DIRTY = 1  # the wave whose straddling column carries NaN, ±Inf and ±0.0


def _straddle(seed):
    """Six Aᵀ waves; in wave w the column STRADDLE[w][0] crosses a chunk edge after STRADDLE[w][1] of its entries (wave 5: a column of 1100
    from the start of its run, across the edges at 512 and 1024).  The columns in front of it fill the run up to its start; those behind
    it have 0-5 entries."""
    rng = np.random.default_rng(seed)
    m = 300
    lens, strad = [], []
    for w, (q, o, after) in enumerate(STRADDLE):
        pre = rng.multinomial(TCH - o, np.ones(q) / q) if q else np.zeros(0, dtype=np.int64)
        lens += list(pre) + [o + after] + list(rng.integers(0, 6, WAVE - q - 1))
        strad.append(WAVE * w + q)
    n = len(lens)
    r, c = _cols_entries(rng, m, np.array(lens))
    clean = [s for w, s in enumerate(strad) if w != STRADDLE_DIRTY]
    fx = _fx("cols_straddle", m, n, rng, _values(_pattern(rng, n, r, c, dirty=(c == strad[STRADDLE_DIRTY]))), {"cols": clean, "rows": np.arange(m)})
    fx.straddlers = strad
    return fx


def _aligned(seed):
    """Two Aᵀ waves of runs longer than 512 in which no column crosses a chunk edge: wave 0 has a column that ends exactly at entry 512 and
    one that starts there; wave 1 starts with a column of exactly 512."""
    rng = np.random.default_rng(seed)
    m = 300
    w0 = [30] * 10 + [212, 300] + list(rng.integers(0, 4, WAVE - 12))
    w1 = [512] + list(rng.integers(0, 6, WAVE - 1))
    lens = np.array(w0 + w1)
    r, c = _cols_entries(rng, m, lens)
    return _fx("cols_aligned", m, len(lens), rng, _values(_pattern(rng, len(lens), r, c)), {"cols": [10, 11, WAVE], "rows": np.arange(m)})


def _mixed(seed):
    """200 x 200 (a partial last slice and a partial last wave): short rows of 2-8, row 70 with 600 more entries (long), column 130 with
    700 more (its wave's run is longer than 512).  A few entries away from row 70 and column 130 carry NaN, ±Inf and ±0.0."""
    rng = np.random.default_rng(seed)
    m = n = 200
    r0, c0 = _rows_entries(rng, n, rng.integers(2, 9, m))
    r = np.concatenate([r0, np.full(600, 70), rng.integers(0, m, 700)])
    c = np.concatenate([c0, rng.integers(0, n, 600), np.full(700, 130)])
    pat = _pattern(rng, n, r, c, dirty=(r != 70) & (c != 130) & (r % 50 == 3))
    return _fx("mixed", m, n, rng, _values(pat), {"rows": np.flatnonzero(~layout(m, n, *pat[:2]).long), "long": [70], "cols": [130]})


def _sized(m, n, seed):
    rng = np.random.default_rng(seed)
    d = 0.2 if max(m, n) < 100 else (0.1 if max(m, n) < 200 else 0.05)
    return _fx(f"size_{m}x{n}", m, n, rng, lambda rng: random_csc(rng, m, n, density=d), {"rows": np.arange(m), "cols": np.arange(n)})


SIZES = ((63, 65), (65, 63), (64, 64), (127, 129), (129, 127), (255, 257), (257, 255), (256, 256))


@functools.lru_cache(maxsize=None)
def fixtures():
    """Every fixture by name (built once per process; deterministic)."""
    fx = [
        _absolute("abs256", 256, 1), _absolute("abs257", 257, 2),
        # a full slice: 63 rows holding 1499 (50 of 24, 13 of 23); mean = ceil((1499 + L) / 64) = 25 for L = 100 and 101
        _relative("rel_full_at", 64, 5, 100, [24] * 50 + [23] * 13, 3), _relative("rel_full_over", 64, 5, 101, [24] * 50 + [23] * 13, 4),
        # the partial last slice of 101 rows (37): 36 rows holding 494 (26 of 14, 10 of 13); mean = ceil((494 + L) / 37) = 15 for L = 60, 61
        _relative("rel_part_at", 101, 84, 60, [14] * 26 + [13] * 10, 5), _relative("rel_part_over", 101, 84, 61, [14] * 26 + [13] * 10, 6),
        _long_rows("long512", 512, 7), _long_rows("long513", 513, 8), _long_rows("long1024", 1024, 9), _long_rows("long1025", 1025, 10),
        _run("run512", 512, 11), _run("run513", 513, 12),
        _aligned(13), _straddle(14), _mixed(15),
    ] + [_sized(m, n, 16 + q) for q, (m, n) in enumerate(SIZES)]
    return {f.name: f for f in fx}


THRESHOLD_FIXTURES = ("abs256", "abs257", "rel_full_at", "rel_full_over", "rel_part_at", "rel_part_over", "long512", "long513", "long1024",
                      "long1025", "run512", "run513", "cols_aligned", "cols_straddle") + tuple(f"size_{m}x{n}" for m, n in SIZES)


def _l(f):
    return layout(f.m, f.n, f.colptr, f.rowval)


def _rowside(t):
    def side(f):
        L = _l(f)
        return bool(L.long[t]), int(L.lens[t] - 4 * L.mean[t // SLICE]), int(L.slice_rows[t // SLICE])
    return side


# threshold: (fixture on one side, fixture on the other, what the mirror reads, its value on each side)
PAIRS = {
    "row length 256 | 257 (absolute rule; 4·mean = 260)": ("abs256", "abs257", lambda f: (bool(_l(f).long[17]), int(_l(f).lens[17]),
                                                                                          int(4 * _l(f).mean[0])), ((False, 256, 260), (True, 257, 260))),
    "4·mean | 4·mean + 1, full slice": ("rel_full_at", "rel_full_over", _rowside(5), ((False, 0, 64), (True, 1, 64))),
    "4·mean | 4·mean + 1, partial last slice": ("rel_part_at", "rel_part_over", _rowside(84), ((False, 0, 37), (True, 1, 37))),
    "long row 512 | 513": ("long512", "long513", lambda f: (bool(_l(f).long[10]), long_chunks(int(_l(f).lens[10]))), ((True, 1), (True, 2))),
    "long row 1024 | 1025": ("long1024", "long1025", lambda f: (bool(_l(f).long[10]), long_chunks(int(_l(f).lens[10]))), ((True, 2), (True, 3))),
    "Aᵀ run 512 | 513": ("run512", "run513", lambda f: (int(_l(f).run[0]), long_chunks(int(_l(f).run[0])), sorted(_l(f).cross)),
                         ((512, 1, []), (513, 2, [63]))),
    "column inside | across a chunk edge": ("cols_aligned", "cols_straddle",
                                            lambda f: sorted((c, tuple(o)) for c, o in _l(f).cross.items()),
                                            ([], sorted((WAVE * w + q, (o,) if w < 5 else (512, 1024)) for w, (q, o, _) in enumerate(STRADDLE)))),
    "rows 63 | 65 (one slice | two)": ("size_63x65", "size_65x63", lambda f: (_l(f).nslices, int(_l(f).slice_rows[-1])), ((1, 63), (2, 1))),
    "rows 64 | 65": ("size_64x64", "size_65x63", lambda f: (_l(f).nslices, int(_l(f).slice_rows[-1])), ((1, 64), (2, 1))),
    "rows 127 | 129": ("size_127x129", "size_129x127", lambda f: (_l(f).nslices, int(_l(f).slice_rows[-1])), ((2, 63), (3, 1))),
    "rows 255 | 257 (one rows workgroup | two)": ("size_255x257", "size_257x255", lambda f: _l(f).row_wgs, (1, 2)),
    "rows 256 | 257": ("size_256x256", "size_257x255", lambda f: _l(f).row_wgs, (1, 2)),
    "columns 63 | 65 (one Aᵀ wave | two)": ("size_65x63", "size_63x65", lambda f: _l(f).waves, (1, 2)),
    "columns 64 | 65": ("size_64x64", "size_63x65", lambda f: _l(f).waves, (1, 2)),
    "columns 127 | 129": ("size_129x127", "size_127x129", lambda f: _l(f).waves, (2, 3)),
    "columns 255 | 257": ("size_257x255", "size_255x257", lambda f: _l(f).waves, (4, 5)),
    "columns 256 | 257": ("size_256x256", "size_255x257", lambda f: _l(f).waves, (4, 5)),
}


# ---- order sensitivity --------------------------------------------------------------------------------------------------------------
def fold(f, path, x, alpha=1.0, reverse=True):
    """The focus elements of `path` for A·x (rows, long) or Aᵀ·x (cols), β = 0, with each element's contributions folded in REVERSED
    storage order -- what a kernel that took them backwards would give (reverse=False: in storage order, the restatement's bits)."""
    cp = np.asarray(f.colptr, dtype=np.int64)
    nnz = int(cp[-1] - 1)
    rv, nz = np.asarray(f.rowval, dtype=np.int64)[:nnz] - 1, np.asarray(f.nzval, dtype=np.float64)[:nnz]
    col = np.repeat(np.arange(f.n), np.diff(cp))
    a = np.float64(alpha)
    out = []
    for e in f.focus[path]:
        if path == "cols":
            terms = nz[cp[e] - 1:cp[e + 1] - 1] * x[rv[cp[e] - 1:cp[e + 1] - 1]]
        else:
            sel = np.flatnonzero(rv == e)
            terms = nz[sel] * (x[col[sel]] * a)
        acc = np.float64(0.0)
        for t in (terms[::-1] if reverse else terms):
            acc = acc + t
        out.append(np.float64(0.0) + acc * a if path == "cols" else acc)
    return np.array(out, dtype=np.float64)


def order_x(f, path):
    """The vector the order check multiplies by: widely spread, no special values."""
    rng = np.random.default_rng(99)
    rows = f.m if path == "cols" else f.n
    return rng.standard_normal(rows) * 10.0 ** rng.integers(-3, 4, rows)


def order_sensitive(f, path):
    x = order_x(f, path)
    want = spmv_ref(f.m, f.n, f.colptr, f.rowval, f.nzval, x, adjoint=(path == "cols"))[f.focus[path]]
    rev = fold(f, path, x)
    return int(np.count_nonzero(bits(want) != bits(rev)))


# ---- above 2^24 ---------------------------------------------------------------------------------------------------------------------
BIG_LONG_ROW = (1 << 24) + 100   # 600 more entries: long
BIG_LONG_COL = (1 << 24) + 150   # 700 more entries: its wave's run crosses a chunk edge


def big_matrix(seed=0):
    """m = n = 2^24 + 197: every column holds its diagonal, its sub-diagonal (row j + 1, wrapping) and a far row (j·7919 + 12345 mod m), in
    that order on even columns and far row first on odd ones; row BIG_LONG_ROW gets one more entry in each of 600 columns, column
    BIG_LONG_COL 700 more (some rows twice), shuffled.  Returns (m, n, colptr, rowval, nzval)."""
    rng = np.random.default_rng(seed)
    N = BIG
    j = np.arange(N, dtype=np.int64)
    base = np.stack([j, (j + 1) % N, (j * 7919 + 12345) % N], axis=1)
    base[1::2] = base[1::2][:, [2, 0, 1]]
    extra_cols = np.unique(rng.integers(0, N, 700))
    extra_cols = rng.permutation(extra_cols[extra_cols != BIG_LONG_COL])[:600]
    cnt = np.full(N, 3, dtype=np.int64)
    cnt[extra_cols] += 1
    cnt[BIG_LONG_COL] += 700
    colptr = np.empty(N + 1, dtype=np.int64)
    colptr[0] = 1
    np.cumsum(cnt, out=colptr[1:])
    colptr[1:] += 1
    rowval = np.empty(int(colptr[-1] - 1), dtype=np.int64)
    start = colptr[:-1] - 1
    for q in range(3):
        rowval[start + q] = base[:, q]
    del base
    rowval[start[extra_cols] + 3] = BIG_LONG_ROW
    s = start[BIG_LONG_COL]
    lc = np.concatenate([rowval[s:s + 3], rng.integers(0, N, 690), rng.integers(0, N, 5).repeat(2)])
    rowval[s:s + 703] = lc[rng.permutation(703)]
    rowval += 1
    nnz = len(rowval)
    nzval = rng.standard_normal(nnz) * 10.0 ** rng.integers(-8, 8, nnz)
    nzval[rng.random(nnz) < 0.05] = -0.0
    return N, N, colptr, rowval, nzval
