"""Inputs for lump_and_spray (csrc/otmb_lump.hip) on which the kernel has something to do: patterns that really connect cells, rows wider than
the sweep's 256 threads, blocks at the 4096-cell limit, and paths on which min-label propagation needs many sweeps.

  neighbour_pattern   a random subset of the 6-neighbour links as a symmetric CSC pattern (or a deliberately one-directional one);
  sweep_case          the inputs of tests/test_lump_and_spray.py::test_lump_and_spray_random_sweep, seed by seed;
  snake_pattern       all cells wet, every bi x bj tile of every level linked along ONE boustrophedon path (or two interleaved ones): a label
                      has to travel the whole path, so lump_components_kernel sweeps its block many times;
  label_sweeps        restates that kernel's loop for one anchor and counts its sweeps and components;
  WIDE_CASES / wide_case   grids whose rows straddle the stride of 256 (LS_THREADS), up to the nx <= 4900 bound, and full blocks.

tests/test_lump_grids_ref.py asserts on the CPU that these inputs are what tests/test_lump_wide.py needs.  numpy alone."""
import numpy as np

LS_THREADS = 256      # threads of lump_sweep_kernel: a row is walked with this stride
NX_MAX = 4900         # otmb_lump_and_spray_plan_dev refuses wider rows (its LDS per row: 13 * nx + 16 bytes)
SWEEP_SEEDS = range(30)


def _csc(cols, N):
    colptr = np.ones(N + 1, dtype=np.int64)
    rowval = []
    for c in range(1, N + 1):
        rows = sorted(cols[c])
        rowval.extend(rows)
        colptr[c] = colptr[c - 1] + len(rows)
    rowval = np.array(rowval, dtype=np.int64)
    return colptr, rowval, np.ones(len(rowval))


def wet_rank(wet):
    """1-based rank of every wet cell in column-major order (0 on dry cells): the row / column of T that belongs to it."""
    N = int(wet.sum())
    rank = np.zeros(wet.shape, dtype=np.int64, order="F")
    flat = rank.reshape(-1, order="F")  # a view, because rank is column-major: of a C-ordered array it is a copy, and the ranks are lost
    flat[wet.reshape(-1, order="F")] = np.arange(1, N + 1)
    assert np.shares_memory(flat, rank) and rank.max() == N
    return rank


def neighbour_pattern(wet, rng, keep=0.7, periodic_i=True, drop_reverse=0.0):
    """T = (colptr, rowval, ones), 1-based N x N: the diagonal and each link to the +i, +j, +k neighbour with probability `keep` (keep >= 1: all
    of them, nothing drawn), symmetric.  drop_reverse > 0 leaves the reverse entry of a link out with that probability: a one-directional pattern,
    which the reference refuses (Graphs.SimpleGraph).  One draw per candidate link, one more per kept link when drop_reverse > 0, cells in
    np.argwhere order."""
    nx, ny, nz = wet.shape
    N = int(wet.sum())
    rank = wet_rank(wet)
    cols = [set([c]) for c in range(N + 1)]
    for (a, b, c) in np.argwhere(wet):
        for (da, db, dc) in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            a2, b2, c2 = a + da, b + db, c + dc
            if periodic_i:
                a2 %= nx
            if a2 < nx and b2 < ny and c2 < nz and wet[a2, b2, c2] and (keep >= 1.0 or rng.random() < keep):
                r1, r2 = int(rank[a, b, c]), int(rank[a2, b2, c2])
                cols[r1].add(r2)
                if not (drop_reverse > 0.0 and rng.random() < drop_reverse):
                    cols[r2].add(r1)
    assert rank.max() == N
    return _csc(cols, N)


def sweep_case(seed):
    """(wet, vol, T, mask, (di, dj, dk)) of the random sweep: small grids, masks, block sizes (blocks larger than the grid and dk > 1 among them);
    every seventh seed from 3 on draws a one-directional pattern."""
    rng = np.random.default_rng(7000 + seed)
    nx, ny, nz = int(rng.integers(1, 14)), int(rng.integers(1, 9)), int(rng.integers(1, 6))
    wet = rng.random((nx, ny, nz)) < rng.uniform(0.3, 1.0)
    if not wet.any():
        wet[0, 0, 0] = True
    N = int(wet.sum())
    broken = seed % 7 == 3
    T = neighbour_pattern(wet, rng, keep=0.7, periodic_i=True, drop_reverse=0.3 if broken else 0.0)
    vol = rng.uniform(1.0, 1e6, N)
    di, dj, dk = int(rng.integers(1, 6)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
    mask = None if rng.random() < 0.3 else (rng.random(wet.shape) < rng.uniform(0.2, 1.0))
    return wet, vol, T, mask, (di, dj, dk)


# ---- snakes: many sweeps of the min-label loop ---------------------------------------------------------------------------------------------------
def snake_path(bi, bj, reverse=False):
    """The cells (a, b) of a bi x bj tile along the boustrophedon: row 0 left to right, row 1 right to left, ...; reverse: row 0 right to left,
    row 1 left to right, ... (the path starts at the tile's cell bi - 1, not at its smallest vertex)."""
    return [(a if (b % 2 == 0) != reverse else bi - 1 - a, b) for b in range(bj) for a in range(bi)]


def snake_pattern(nx, ny, nz, bi, bj, reverse=False, two=False):
    """(wet, T): all cells wet; inside every bi x bj tile of every level (tiles start at multiples of bi, bj and are cut at the grid's edge) the
    cells are linked only along snake_path, position a with a + 1 (two: with a + 2, two interleaved components per tile)."""
    wet = np.ones((nx, ny, nz), dtype=bool)
    N = nx * ny * nz
    rank = wet_rank(wet)
    cols = [set([c]) for c in range(N + 1)]
    step = 2 if two else 1
    for k in range(nz):
        for j0 in range(0, ny, bj):
            for i0 in range(0, nx, bi):
                w, h = min(bi, nx - i0), min(bj, ny - j0)
                path = snake_path(w, h, reverse)
                for q in range(len(path) - step):
                    (a, b), (a2, b2) = path[q], path[q + step]
                    r1, r2 = int(rank[i0 + a, j0 + b, k]), int(rank[i0 + a2, j0 + b2, k])
                    cols[r1].add(r2)
                    cols[r2].add(r1)
    return wet, _csc(cols, N)


def label_sweeps(wet, T, anchor, block):
    """(sweeps, components) of lump_components_kernel's loop for the block anchored at `anchor`: the block's wet cells start with their local
    index as label, the cells are visited in block order (a fastest), each takes the smallest label among itself and the cells of its column of T
    that lie inside the block, labels are updated IN PLACE, and sweeps are repeated until one changes nothing (that last one is counted)."""
    nx, ny, nz = wet.shape
    (ai, aj, ak), (di, dj, dk) = anchor, block
    colptr, rowval, _ = T
    rank = wet_rank(wet)
    lwet = np.flatnonzero(wet.reshape(-1, order="F"))  # 0-based linear index of every wet rank

    def local(L):
        a, b, c = L % nx - ai, (L // nx) % ny - aj, L // (nx * ny) - ak
        return (c * dj + b) * di + a if (0 <= a < di and 0 <= b < dj and 0 <= c < dk) else -1

    lab, nbr = {}, {}
    for c in range(dk):
        for b in range(dj):
            for a in range(di):
                if ai + a < nx and aj + b < ny and ak + c < nz and wet[ai + a, aj + b, ak + c]:
                    l = (c * dj + b) * di + a
                    col = int(rank[ai + a, aj + b, ak + c])
                    lab[l] = l
                    nbr[l] = [l2 for l2 in (local(int(lwet[r - 1])) for r in rowval[colptr[col - 1] - 1: colptr[col] - 1]) if l2 >= 0]
    sweeps, changed = 0, True
    while changed:
        changed = False
        sweeps += 1
        for l in sorted(lab):
            best = min([lab[l]] + [lab[l2] for l2 in nbr[l]])
            if best < lab[l]:
                lab[l] = best
                changed = True
    return sweeps, len(set(lab.values()))


SNAKE_GRID = (40, 20, 2)
SNAKE_CASES = [  # (tile, keywords of snake_pattern, block)
    ((16, 16), dict(), (16, 16, 1)),
    ((16, 16), dict(reverse=True), (16, 16, 1)),
    ((16, 16), dict(two=True), (16, 16, 1)),
    ((8, 8), dict(), (16, 16, 2)),                 # eight components per anchor
]
_snakes = {}


def snake_case(q):
    """(wet, vol, T, block) of SNAKE_CASES[q] on SNAKE_GRID; built once and left unchanged."""
    if q not in _snakes:
        (bi, bj), kw, block = SNAKE_CASES[q]
        wet, T = snake_pattern(*SNAKE_GRID, bi, bj, **kw)
        vol = np.random.default_rng(9500 + q).uniform(1.0, 1e6, int(wet.sum()))
        _snakes[q] = (wet, vol, T, block)
    return _snakes[q]


# ---- wide rows, blocks across the stride, the nx bound, full blocks ---------------------------------------------------------------------------------
WIDE_CASES = [  # (shape, (di, dj, dk))
    ((255, 3, 2), (1, 1, 1)), ((255, 3, 2), (2, 2, 1)),      # rows round the stride of 256: chains of up to nx anchors
    ((256, 3, 2), (1, 1, 1)), ((256, 3, 2), (2, 2, 1)),
    ((257, 3, 2), (1, 1, 1)), ((257, 3, 2), (2, 2, 1)),
    ((513, 3, 1), (1, 2, 1)),
    ((300, 4, 3), (3, 2, 2)),
    ((513, 3, 2), (255, 1, 2)),                              # blocks that straddle the stride
    ((513, 3, 2), (257, 2, 1)),
    ((770, 3, 1), (300, 3, 1)),
    ((600, 8, 1), (512, 8, 1)),                              # a 4096-cell block on a wide row
    ((1000, 2, 2), (7, 2, 2)),                               # many anchors with dk > 1
    ((4900, 2, 1), (1, 1, 1)),                               # the nx bound
    ((4900, 2, 2), (5, 2, 2)),
    ((70, 70, 2), (64, 64, 1)),                              # full blocks
    ((40, 40, 20), (16, 16, 16)),
]
WIDE_MASKS = ("none", "sparse", "dense")
_wide = {}


def wide_id(q):
    shape, block = WIDE_CASES[q]
    return "x".join(map(str, shape)) + "-" + "x".join(map(str, block))


def wide_case(q):
    """(wet, vol, T, masks, block) of WIDE_CASES[q], seed 9000 + q: 80 % wet, neighbour_pattern, volumes uniform on [1, 1e6]; masks: "none" -> None,
    "sparse" -> 15 % of the cells in the mask (irregular free cells, long jumps of the chain), "dense" -> 90 %.  Built once and left unchanged."""
    if q not in _wide:
        shape, block = WIDE_CASES[q]
        rng = np.random.default_rng(9000 + q)
        wet = rng.random(shape) < 0.8
        T = neighbour_pattern(wet, rng)
        vol = rng.uniform(1.0, 1e6, int(wet.sum()))
        masks = {"none": None, "sparse": rng.random(shape) < 0.15, "dense": rng.random(shape) < 0.9}
        for a in (wet, vol, masks["sparse"], masks["dense"]) + T:
            a.setflags(write=False)
        _wide[q] = (wet, vol, T, masks, block)
    return _wide[q]


def first_row_anchors(mask, shape, block):
    """For di = 1: the most anchors any first row of a level holds, from the inputs alone.  Row 0 of a level is covered by no earlier row, and with
    dk = 1 by no earlier level; with di = 1 every free in-mask cell of it is an anchor."""
    nx, ny, nz = shape
    assert block[0] == 1 and block[2] == 1
    return nx if mask is None else int(mask[:, 0, :].sum(axis=0).max())
