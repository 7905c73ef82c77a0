"""CPU: the inputs of tests/lump_grids.py are what the GPU tests of lump_and_spray need -- patterns that connect cells (the random sweep once
handed the device nothing but identity patterns: its cell ranks were assigned through a copy and stayed zero), one-directional patterns where the
sweep expects a refusal, rows of more than 256 anchors, masks that change the result, blocks that need many label sweeps.  The oracle is compared
with its transliteration wherever that is affordable.  numpy and the oracle alone."""
import numpy as np
import pytest

import lump_grids as lg
from oracle import pyref

REFUSED = {10, 17, 24}       # seeds of the sweep with a one-directional link inside a block (seed 3 draws one too, but a 1 x 1 x 1 block)
PYREF_BLOCK, PYREF_N = 600, 12000  # the transliteration is quadratic in the block and walks Python lists: affordable below these


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0] + a[1] + (a[2],), b[0] + b[1] + (b[2],)))


def test_neighbour_pattern_links_cells():
    rng = np.random.default_rng(1)
    wet = rng.random((5, 4, 3)) < 0.8
    colptr, rowval, _ = lg.neighbour_pattern(wet, rng)
    N = int(wet.sum())
    assert len(colptr) == N + 1 and colptr[-1] - 1 == len(rowval) > 2 * N  # far more than a diagonal
    assert rowval.min() == 1 and rowval.max() == N
    cols = np.repeat(np.arange(1, N + 1), np.diff(colptr))
    assert set(zip(rowval, cols)) == set(zip(cols, rowval))                 # symmetric
    c2, r2, _ = lg.neighbour_pattern(wet, np.random.default_rng(2), drop_reverse=0.5)
    k2 = np.repeat(np.arange(1, N + 1), np.diff(c2))
    assert set(zip(r2, k2)) != set(zip(k2, r2))                             # one-directional on request


def test_sweep_seeds_lump_and_three_are_refused(oracle):
    """What test_lump_and_spray_random_sweep rests on: its ASYMMETRIC_PATTERN branch is taken by seeds 10, 17 and 24 and by no other, most of the
    other seeds really merge cells, and the oracle is its transliteration's equal on all of them."""
    refused, lumping = set(), 0
    for seed in lg.SWEEP_SEEDS:
        wet, vol, T, mask, (di, dj, dk) = lg.sweep_case(seed)
        assert T[1].max() == len(vol) and len(T[1]) >= len(vol)
        try:
            a = oracle.lump_and_spray(wet, vol, T, mask, di, dj, dk)
        except oracle.OracleError:
            refused.add(seed)
            with pytest.raises(pyref.AsymmetricConnectivity):
                pyref.lump_and_spray(wet, vol, T, mask, di, dj, dk)
            continue
        assert _equal(a, pyref.lump_and_spray(wet, vol, T, mask, di, dj, dk)), seed
        lumping += len(a[2]) < len(vol)
    assert refused == REFUSED
    assert lumping >= 20


@pytest.mark.parametrize("q", range(len(lg.WIDE_CASES)), ids=lg.wide_id)
def test_wide_cases_lump_and_masks_matter(oracle, q):
    wet, vol, T, masks, block = lg.wide_case(q)
    shape = lg.WIDE_CASES[q][0]
    N, bv = len(vol), block[0] * block[1] * block[2]
    assert wet.shape == shape and shape[0] <= lg.NX_MAX and bv <= 4096
    got = {m: oracle.lump_and_spray(wet, vol, T, masks[m], *block) for m in lg.WIDE_MASKS}
    Nc = {m: len(got[m][2]) for m in lg.WIDE_MASKS}
    if bv > 1:
        assert Nc["none"] < N                                   # cells are merged
        assert Nc["sparse"] > Nc["dense"]                       # and the mask decides how many
    else:
        assert Nc["none"] == N
    if block[0] == 1 and block[2] == 1 and shape[0] > lg.LS_THREADS:
        assert lg.first_row_anchors(masks["none"], shape, block) > lg.LS_THREADS  # a chain of more anchors than the sweep has threads
        if 0.8 * shape[0] > lg.LS_THREADS:                      # ... with an irregular mask too, where 90 % of the row leaves that many
            assert lg.first_row_anchors(masks["dense"], shape, block) > lg.LS_THREADS
    if bv <= PYREF_BLOCK and N < PYREF_N:
        for m in lg.WIDE_MASKS:
            assert _equal(got[m], pyref.lump_and_spray(wet, vol, T, masks[m], *block)), m


def test_wide_cases_are_the_listed_ones():
    """The rows round the stride, the blocks across it, the bound and the full blocks are all there."""
    cases = set(lg.WIDE_CASES)
    for nx in (255, 256, 257):
        assert ((nx, 3, 2), (1, 1, 1)) in cases and ((nx, 3, 2), (2, 2, 1)) in cases
    assert any(s[0] == lg.NX_MAX and b[2] == 1 for s, b in cases) and any(s[0] == lg.NX_MAX and b[2] > 1 for s, b in cases)
    assert sum(b[0] * b[1] * b[2] == 4096 for s, b in cases) == 3
    assert any(b[0] > lg.LS_THREADS and s[0] > 2 * lg.LS_THREADS for s, b in cases)
    assert lg.NX_MAX * 13 + 16 == 63716 <= 65536                        # the sweep's LDS at the bound: close below 64 KiB


@pytest.mark.parametrize("q", range(len(lg.SNAKE_CASES)))
def test_snakes_need_many_sweeps(oracle, q):
    """A label travels a whole left-to-right row of the path in one in-place sweep, but only one cell per sweep along a right-to-left row: a bi x bj
    snake needs 1 + (bi - 1) * (bj // 2) sweeps that change something and one that does not.  A 6-neighbour stencil needs two to four."""
    wet, vol, T, block = lg.snake_case(q)
    (bi, bj), kw, _ = lg.SNAKE_CASES[q]
    sweeps, comps = lg.label_sweeps(wet, T, (0, 0, 0), (bi, bj, 1))   # the first tile
    assert comps == (2 if kw.get("two") else 1)
    if not kw:
        assert sweeps == 2 + (bi - 1) * (bj // 2)
    if (bi, bj) == (16, 16):
        assert sweeps >= 50
    else:
        assert lg.label_sweeps(wet, T, (0, 0, 0), block)[1] == 8      # four tiles on each of two levels in the anchor's block
    a = oracle.lump_and_spray(wet, vol, T, None, *block)
    assert _equal(a, pyref.lump_and_spray(wet, vol, T, None, *block))
    nx, ny, nz = wet.shape
    tiles = -(-nx // bi) * -(-ny // bj) * nz
    assert len(a[2]) == tiles * (2 if kw.get("two") else 1)             # no block merges two tiles
