"""lump_and_spray (csrc/otmb_lump.hip) against the oracle where its kernels have the most to get wrong (tests/lump_grids.py; run with -m gpu):
rows wider than the sweep's 256 threads (the second stride of every row loop, chains of up to 4900 anchors and thirteen rounds of pointer
doubling), blocks that straddle the stride, the nx <= 4900 bound with its 63 716 bytes of LDS, blocks of 4096 cells, paths on which the min-label
loop of one thread sweeps its block more than a hundred times, several interleaved components per block, and the device entry points with a
device mask on a tripolar T whose rows are 328 wide.  Everything bit for bit; tests/test_lump_grids_ref.py asserts on the CPU that the inputs are
what these tests count on."""
import numpy as np
import pytest

import lump_grids as lg
import mid_grids as mg
from test_lump_and_spray import _same
from test_oracle import lump_mask

pytestmark = pytest.mark.gpu


def _api_T(T):
    import otmb_amd.api as api

    N = len(T[0]) - 1
    return api.SparseMatrixCSC(N, N, *T)


@pytest.mark.parametrize("q", range(len(lg.WIDE_CASES)), ids=lg.wide_id)
def test_wide_rows_and_full_blocks_match_the_oracle(oracle, q):
    import otmb_amd.api as api

    wet, vol, T, masks, (di, dj, dk) = lg.wide_case(q)
    Tm = _api_T(T)
    for m in lg.WIDE_MASKS:
        want = oracle.lump_and_spray(wet, vol, T, masks[m], di, dj, dk)
        got = api.lump_and_spray(wet, vol, Tm, masks[m], di=di, dj=dj, dk=dk)
        _same(got, want, (lg.wide_id(q), m))


@pytest.mark.parametrize("q", range(len(lg.SNAKE_CASES)))
def test_snakes_match_the_oracle(oracle, q):
    """Many sweeps of the label loop (122, 107, 58 for the 16 x 16 tiles), two interleaved components per tile, eight components per anchor."""
    import otmb_amd.api as api

    wet, vol, T, (di, dj, dk) = lg.snake_case(q)
    want = oracle.lump_and_spray(wet, vol, T, None, di, dj, dk)
    got = api.lump_and_spray(wet, vol, _api_T(T), None, di=di, dj=dj, dk=dk)
    _same(got, want, ("snake", q))


def test_asymmetric_wide_pattern_is_refused_and_the_context_goes_on(oracle):
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    q = lg.WIDE_CASES.index(((513, 3, 2), (257, 2, 1)))
    wet, vol, T, masks, (di, dj, dk) = lg.wide_case(q)
    bad = lg.neighbour_pattern(wet, np.random.default_rng(9900), drop_reverse=0.3)
    with pytest.raises(oracle.OracleError, match="symmetric"):
        oracle.lump_and_spray(wet, vol, bad, None, di, dj, dk)
    with pytest.raises(OtmbError) as e:
        api.lump_and_spray(wet, vol, _api_T(bad), None, di=di, dj=dj, dk=dk)
    assert e.value.name == "ASYMMETRIC_PATTERN"
    want = oracle.lump_and_spray(wet, vol, T, None, di, dj, dk)
    _same(api.lump_and_spray(wet, vol, _api_T(T), None, di=di, dj=dj, dk=dk), want, "symmetric, after the refusal")


def test_nx_bound_and_one_past_it(oracle):
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    nx = lg.NX_MAX + 1
    wet = np.ones((nx, 2, 1), dtype=bool)
    N = wet.size
    eye = api.SparseMatrixCSC(N, N, np.arange(1, N + 2, dtype=np.int64), np.arange(1, N + 1, dtype=np.int64), np.ones(N))
    with pytest.raises(OtmbError, match="nx <= 4900") as e:
        api.lump_and_spray(wet, np.ones(N), eye, None, di=1, dj=1, dk=1)
    assert e.value.name == "INVALID_ARG"
    q = lg.WIDE_CASES.index(((lg.NX_MAX, 2, 1), (1, 1, 1)))
    wet, vol, T, masks, (di, dj, dk) = lg.wide_case(q)
    for m in lg.WIDE_MASKS:
        want = oracle.lump_and_spray(wet, vol, T, masks[m], di, dj, dk)
        _same(api.lump_and_spray(wet, vol, _api_T(T), masks[m], di=di, dj=dj, dk=dk), want, ("at the bound", m))


def test_coarsen_with_the_oracles_operators_of_a_wide_case(oracle):
    """The chain LUMP * T * SPRAY on a 300-wide row, with LUMP and SPRAY from the oracle: an input the device had no part in."""
    import otmb_amd.api as api
    from spmatmul_ref import coarse_ref
    from test_coarsen import _same as same_csc

    q = lg.WIDE_CASES.index(((300, 4, 3), (3, 2, 2)))
    wet, vol, T, masks, (di, dj, dk) = lg.wide_case(q)
    rL, rS, rvc = oracle.lump_and_spray(wet, vol, T, masks["dense"], di, dj, dk)
    N, Nc = len(vol), len(rvc)
    L, S = api.SparseMatrixCSC(Nc, N, *rL), api.SparseMatrixCSC(N, Nc, *rS)
    values = np.random.default_rng(9901).standard_normal(len(T[1]))
    Tm = api.SparseMatrixCSC(N, N, T[0], T[1], values)
    same_csc(api.coarsen(L, Tm, S), coarse_ref(L, Tm, S), "300x4x3, dense mask")


# ---- the device entry points on a tripolar T with rows of 328 cells ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid(oracle):
    """The mid grid after one step (T resident), with the oracle's wet mask, volumes and T."""
    from mid_grids_worker import assembler, dev

    g, gm = mg.case("mid")
    idx = mg.indices(oracle, "mid")
    wet = idx["wet3D"].astype(bool)
    vol = np.asarray(gm.v3D).reshape(-1, order="F")[wet.reshape(-1, order="F")]
    T = mg.reference(oracle, "mid", "base")["T"]
    asm = assembler("mid")
    u, v, fill = mg.field("mid", "base")
    asm.step(dev(u), dev(v), fill)
    yield asm, wet, vol, T
    del asm


@pytest.mark.parametrize("block", [(2, 2, 1), (5, 3, 2), (40, 2, 1), (257, 1, 1), (16, 16, 2)], ids=lambda b: "x".join(map(str, b)))
def test_device_entry_points_on_the_mid_grid(oracle, mid, block):
    """otmb_lump_and_spray_plan_dev / fill_dev on resident arrays: without a mask and with a device mask; with dk > 1 one workgroup carries the
    covered levels across all 17 of them on rows of 328 cells."""
    from mid_grids_worker import dev

    asm, wet, vol, T = mid
    di, dj, dk = block
    for m in (None, lump_mask(wet, 5)):
        want = oracle.lump_and_spray(wet, vol, T, m, di, dj, dk)
        dm = None if m is None else dev(m.astype(np.uint8))
        L, S, vc = asm.lump_and_spray(dm, di, dj, dk)
        for got, ref, nm in ((L[0], want[0][0], "LUMP.colptr"), (L[1], want[0][1], "LUMP.rowval"), (L[2], want[0][2], "LUMP.nzval"),
                             (S[0], want[1][0], "SPRAY.colptr"), (S[1], want[1][1], "SPRAY.rowval"), (S[2], want[1][2], "SPRAY.nzval"),
                             (vc, want[2], "vol_c")):
            got = got.cpu().numpy()
            assert got.shape == ref.shape and np.array_equal(got, ref), (block, m is not None, nm)
