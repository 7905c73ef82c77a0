"""CPU: the fixtures of tests/spmv_edges.py land where they claim.  For every layout threshold of the resident sparse operator there is a
pair of fixtures that the mirror of the layout rule puts on opposite sides; every fixture's focus elements tell a reversed fold from the
storage-order one of tests/spmv_ref.py; the special values sit where the GPU tests (tests/test_spmv_edges.py) need them."""
import numpy as np
import pytest

import spmv_edges as E
from spmv_ref import bits, spmv_ref


@pytest.mark.parametrize("threshold", list(E.PAIRS))
def test_each_threshold_has_a_fixture_on_either_side(threshold):
    a, b, side, (want_a, want_b) = E.PAIRS[threshold]
    F = E.fixtures()
    got = (side(F[a]), side(F[b]))
    assert got == (want_a, want_b), (threshold, got)
    assert got[0] != got[1]


def test_the_threshold_tests_run_exactly_the_paired_fixtures():
    assert {f for a, b, _, _ in E.PAIRS.values() for f in (a, b)} == set(E.THRESHOLD_FIXTURES)
    assert set(E.THRESHOLD_FIXTURES) < set(E.fixtures())


def test_the_mirror_agrees_with_each_fixtures_focus():
    """Focus rows of the "long" path are long, those of "rows" short; the straddling columns are the ones that cross a chunk edge."""
    for f in E.fixtures().values():
        L = E.layout(f.m, f.n, f.colptr, f.rowval)
        for p, e in f.focus.items():
            assert len(e) and e.min() >= 0 and e.max() < (f.n if p == "cols" else f.m), (f.name, p)
        if "long" in f.focus:
            assert L.long[f.focus["long"]].all(), f.name
        if "rows" in f.focus:
            assert not L.long[f.focus["rows"]].any(), f.name
    s = E.fixtures()["cols_straddle"]
    assert sorted(E.layout(s.m, s.n, s.colptr, s.rowval).cross) == s.straddlers
    mixed = E.fixtures()["mixed"]
    L = E.layout(mixed.m, mixed.n, mixed.colptr, mixed.rowval)
    assert L.long.sum() == 1 and L.run.max() > E.TCH and mixed.m % E.SLICE and mixed.n % E.WAVE  # (the tracer-split fixture)


def test_tracer_counts_reach_both_sides_of_each_tracer_threshold():
    """k on the long-row path: a partial group of 64 lanes (63), a full one (64, 128) and one lane of the next (65, 129).  k = 1 ... 17
    and 24 split into register blocks of 8, 4, 2 and 1 in every way: each tail of 4 / 2 / 1 blocks, behind none to three blocks of 8."""
    assert {k: (E.tracer_groups(k), (k - 1) % E.GROUP + 1) for k in E.K_LONG} == {63: (1, 63), 64: (1, 64), 65: (2, 1), 128: (2, 64),
                                                                                   129: (3, 1)}
    assert all(sum(E.tracer_blocks(k)) == k for k in E.K_SPLITS)
    tails = {tuple(b for b in E.tracer_blocks(k) if b != 8) for k in E.K_SPLITS}
    assert tails == {tuple(E.tracer_blocks(r)) for r in range(8)}
    assert {E.tracer_blocks(k).count(8) for k in E.K_SPLITS} == {0, 1, 2, 3}
    assert E.tracer_blocks(15) == [8, 4, 2, 1] and E.K_BASE == (1, 3, 8)


@pytest.mark.parametrize("name", sorted(E.fixtures()))
def test_every_fixture_is_order_sensitive_on_every_path_it_targets(name):
    """As test_spmv_ref.test_a_reordered_sum_differs_in_the_last_bit: in at least one focus element of each path, the restatement differs
    from the same contributions folded in reversed order -- a fixture that cannot tell the two apart would not catch a reordered fold.
    Folded forwards, the same terms give the restatement's bits on every focus element (the difference is the order's alone)."""
    f = E.fixtures()[name]
    for path in f.focus:
        x = E.order_x(f, path)
        want = spmv_ref(*f.A, x, adjoint=(path == "cols"))[f.focus[path]]
        assert np.array_equal(bits(E.fold(f, path, x, reverse=False)), bits(want)), (name, path)
        assert E.order_sensitive(f, path) > 0, (name, path)


def _specials(v):
    return {"+0": bool(np.any((v == 0) & ~np.signbit(v))), "-0": bool(np.any((v == 0) & np.signbit(v))), "nan": bool(np.any(np.isnan(v))),
            "+inf": bool(np.any(v == np.inf)), "-inf": bool(np.any(v == -np.inf))}


def test_special_values_duplicates_and_unsorted_rows():
    """A long row and an Aᵀ column across a chunk edge hold stored +0.0, -0.0, NaN, +Inf and -Inf, and a duplicate (the row twice in one
    column); the column also unsorted rows.  Every fixture has duplicate and unsorted rows and stored ±0.0."""
    F = E.fixtures()
    for name in ("long512", "long513", "long1024", "long1025"):
        f = F[name]
        col = np.repeat(np.arange(f.n), np.diff(f.colptr))
        sel = f.rowval == 130  # (row 129, 0-based)
        assert E.layout(f.m, f.n, f.colptr, f.rowval).long[129], name
        assert all(_specials(f.nzval[sel]).values()), (name, _specials(f.nzval[sel]))
        assert len(np.unique(col[sel])) < sel.sum(), name
    s = F["cols_straddle"]
    c = s.straddlers[E.STRADDLE_DIRTY]
    assert c in E.layout(s.m, s.n, s.colptr, s.rowval).cross
    r, v = s.rowval[s.colptr[c] - 1:s.colptr[c + 1] - 1], s.nzval[s.colptr[c] - 1:s.colptr[c + 1] - 1]
    assert all(_specials(v).values()) and len(set(r)) < len(r) and np.any(np.diff(r) < 0), _specials(v)
    for f in F.values():
        col = np.repeat(np.arange(f.n), np.diff(f.colptr))
        key = col * (f.m + 1) + f.rowval
        assert len(np.unique(key)) < len(key), (f.name, "duplicates")
        assert np.any((np.diff(f.rowval) < 0) & (np.diff(col) == 0)), (f.name, "unsorted")
        sp = _specials(f.nzval)
        assert sp["+0"] and sp["-0"], (f.name, sp)


def test_the_matrix_above_2_24():
    """m = n = 2^24 + 197: more rows and columns than SP_GRID's 2^24 threads (the plan's per-row and per-column loops go round twice), a
    partial last slice, one long row and one column of more than 512 entries across a chunk edge, both at indices above 2^24."""
    m, n, p, i, v = E.big_matrix()
    assert m == n == E.BIG and n > E.PLAN_THREADS and p[-1] - 1 == len(i) == len(v)
    assert np.all(np.diff(p) >= 3) and i.min() >= 1 and i.max() <= m
    L = E.layout(m, n, p, i)
    assert L.slice_rows[-1] == 5
    assert list(np.flatnonzero(L.long)) == [E.BIG_LONG_ROW] and 590 < L.lens[E.BIG_LONG_ROW] < 620
    assert E.BIG_LONG_ROW > 1 << 24 and E.BIG_LONG_COL > 1 << 24
    c = E.BIG_LONG_COL
    assert p[c + 1] - p[c] > E.TCH and c in L.cross
    r = i[p[c] - 1:p[c + 1] - 1]
    assert len(set(r)) < len(r) and np.any(np.diff(r) < 0)
    assert np.any(np.diff(i[:6]) < 0)  # (odd columns store their far row first)
