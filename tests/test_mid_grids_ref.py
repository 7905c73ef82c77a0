"""CPU: the grids and fields of tests/mid_grids.py are what tests/test_mid_grids.py needs -- more than one scan group, a seam row that goes round
the XCDs, tiles of a few rows, exact cancellations in quantity, the sorted placement of the synthetic sparse() call.  Stated as inequalities: a
later change to synthetic.make_grid may move the counts, but must not be able to turn the GPU tests into one-group tests unnoticed.
numpy and the oracle alone."""
import numpy as np

import mid_grids as mg

CUS = 256          # compute units of the MI355X: the pair kernel of facefluxes is taken where ceil(P / 32) <= 16 * CUs
XCDS = 8


def test_mid_grid_spans_two_scan_groups_and_tiles_of_a_few_rows(oracle):
    nx, ny, nz = mg.SHAPES["mid"]
    idx = mg.indices(oracle, "mid")
    N = idx["N"]
    assert N == int(mg.wet_mask("mid").sum())
    group_cols = mg.TILE * mg.SCAN_GROUP
    assert group_cols < N < 2 * group_cols                      # the second scan group of the fill pass, of spadd and of sparse()
    ntiles = mg.fill_tiles(N)
    assert mg.scan_groups(ntiles) == 2
    last = ntiles - mg.SCAN_GROUP * (mg.scan_groups(ntiles) - 1)
    assert 64 <= last < mg.SCAN_GROUP                           # a partial last group, of more than one wave of tiles
    rows, seam = mg.tile_rows("mid")
    assert seam.sum() > XCDS                                    # the round-robin deal of the heavy tiles goes round
    assert seam[: mg.SCAN_GROUP].any() and seam[mg.SCAN_GROUP:].any()  # ... with heavy tiles in both groups
    assert rows.mean() < 4                                      # south / north neighbours mostly lie in other tiles
    assert nz % 2 == 1 and nz > 8                               # odd, not a multiple of the chunk of levels a wave marches
    assert -(-nx * ny // 32) * 2 < 16 * CUS                     # far below the pair kernel's limit: ctx.ff_pairs() == 1 on the GPU


def test_mid_grid_fields_cancel_where_they_should(oracle):
    for which in ("plain0", "plain1", "cancel"):
        u, v, fill = mg.field("mid", which)
        wet = mg.wet_mask("mid")
        assert (u[~wet] == fill).all() and (v[~wet] == fill).all()
        assert ((u[wet] == 0).any() or (v[wet] == 0).any()) == (which == "cancel")
    cancel = mg.reference(oracle, "mid", "cancel", kap="noH", upwind=False)
    union = mg.union_nnz(cancel)
    assert len(cancel["T"][1]) < union                          # cancellations ...
    assert union - len(cancel["T"][1]) > 100000                 # ... in quantity, and in both scan groups
    short = np.flatnonzero(np.diff(cancel["T"][0]) < mg.union_colptr(cancel))
    assert (short < mg.TILE * mg.SCAN_GROUP).any() and (short >= mg.TILE * mg.SCAN_GROUP).any()
    for which in ("plain0", "plain1"):
        plain = mg.reference(oracle, "mid", which, kap="noH", upwind=False)
        assert len(plain["T"][1]) == mg.union_nnz(plain) == union  # the reserved pattern is a grid constant, and a plain field fills it
    # the stepped fields differ from step to step: other signs, so other upwind patterns of Tadv
    a, b = (mg.reference(oracle, "mid", f"step{k}") for k in (0, 1))
    assert not np.array_equal(a["Tadv"][1], b["Tadv"][1])
    u32, v32, fill32 = mg.field("mid", "f32")
    assert u32.dtype == np.float32 and fill32 == float(np.float32(mg.fill_value("mid"))) and (u32[~mg.wet_mask("mid")] == np.float32(fill32)).all()


def test_wide_grid_spans_the_scan_groups_of_makeindices_and_tfix(oracle):
    nx, ny, nz = mg.SHAPES["wide"]
    idx = mg.indices(oracle, "wide")
    N, G = idx["N"], nx * ny * nz
    assert N > 1048576 + 1024                                   # tfix: a second scan group of 1024-column tiles, of more than one tile
    assert G / mg.BIG_TILE > 2 * mg.SCAN_GROUP                  # makeindices: three scan groups of 1024-cell tiles
    assert mg.scan_groups(-(-G // mg.BIG_TILE)) == 3 and mg.scan_groups(-(-N // mg.BIG_TILE)) == 2
    assert mg.scan_groups(mg.fill_tiles(N)) >= 4                # the fill pass adds several group bases
    assert nx * ny >= 1 << 19 and nx >= 512                     # ff_rows_for: the four-row geometry by itself
    c = mg.reference(oracle, "wide", "cancel", kap="noH", upwind=False)
    short = np.flatnonzero(np.diff(c["T"][0]) < mg.union_colptr(c))
    assert (short < 1048576).sum() > 1000 and (short >= 1048576).sum() > 1000  # tfix moves entries in both of its scan groups


def test_sparse_triplets_sit_where_the_heads_kernel_can_go_wrong():
    I, J, V, facts = mg.sparse_triplets()
    mg.check_sparse_triplets(I, J, V, facts)
    assert len({facts[k] for k in facts}) == 4
