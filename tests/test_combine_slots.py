"""GPU: otmb_op_combine_slots (csrc/otmb_combine.hip): slot dst = Σ_s w_s·(slot s) on the device.  After the call, A·X, Aᵀ·X and a solve on slot
dst have THE BITS of a fresh operator given set_values(combine_ref(...)) -- tests/periodic_pc_ref.py's fold of the slots' nzvals -- which
reads both value arrays of the slot (the row layout for A·X, the CSC copy for Aᵀ·X, both in the solver); the other slots keep their bits.

Operators: solve_ref.dominant(257) with random lines (short-row slices with padding) and solve_ref.arrow(600) (a long row), the builders of
tests/test_op_padded_dev.py; and tiny_tripolar's T cut to nnz = 2048, 2049 and 2050: the kernel gives a workgroup CB_SPAN = 2048 entries,
lane t the entry pairs t, t + 256, ..., so these are one workgroup exactly full, a second workgroup of one entry (an odd count: the last
entry goes alone, not as a 16-byte pair) and a second workgroup of one pair.  Weights (0.25, 0, 0.75) -- a zero weight in the middle -- and
(1/3, 1/3, 1/3) over the tests' three slots, into a fourth slot and into slot 0, a source.  16 and 17 slots: the last count whose pointers and
weights travel as kernel arguments, and the first that reads them from the device table."""
import numpy as np
import pytest

import periodic_pc_ref as PC
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _csc, _operator, _same_bits, _start

pytestmark = pytest.mark.gpu

CB_SPAN = 2048  # csrc/otmb_combine.hip
RTOL, MAXITER = 1e-10, 5000
WEIGHTS = [(0.25, 0.0, 0.75), (1 / 3, 1 / 3, 1 / 3)]


def _cut(p, i, v, nnz):
    """The CSC arrays with the last stored off-diagonal entries dropped until nnz are left (the diagonal stays: the solve needs it)."""
    n = len(p) - 1
    col = np.repeat(np.arange(1, n + 1), np.diff(p))
    off = np.flatnonzero(i != col)
    keep = np.ones(len(v), dtype=bool)
    keep[off[len(off) - (len(v) - nnz):]] = False
    assert keep.sum() == nnz
    p2 = np.concatenate(([1], 1 + np.cumsum(np.bincount(col[keep] - 1, minlength=n)))).astype(np.int64)
    return p2, i[keep], v[keep]


_SYSTEMS = {}


def _system(oracle, which):
    """(n, (colptr, rowval, nzval), lines or None, d, σ, precond) of a case."""
    if which not in _SYSTEMS:
        if which == "dominant":
            _SYSTEMS[which] = (257, R.dominant(257), LR.random_lines(257, 3), np.random.default_rng(13).uniform(0.0, 1.0, 257), 0.5, "lines")
        elif which == "arrow":
            i = R.arrow(600)[1]
            assert np.bincount(i - 1, minlength=600).max() > 512  # a long row of two LDS chunks
            _SYSTEMS[which] = (600, R.arrow(600), None, None, 0.0, "jacobi")
        else:
            T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
            arrays = _cut(*T, int(which))
            assert len(arrays[2]) == int(which)
            _SYSTEMS[which] = (N, arrays, nxt, R.shift("age", N, nsurf)[0], 1.0 / SR.MONTH, "lines")
    return _SYSTEMS[which]


def _reads(D, X, B, d, sigma, precond):
    """What a slot's two value arrays give: A·X (the row layout), Aᵀ·X (the CSC copy), a solve and its adjoint (both) with their reports."""
    out = [D.mul(X), D.mul(X, adjoint=True)]
    for adjoint in (False, True):
        Y, info = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
        assert info.converged.all(), info
        out += [Y, info.iterations.astype(np.float64), info.relres]
    return out


def _fresh(n, p, i, values, nxt):
    import otmb_amd.api as api

    E = api.DeviceOperator(_csc(n, p, i, values))
    if nxt is not None:
        E.set_lines(nxt)
    return E


@pytest.mark.parametrize("dst", [3, 0], ids=["into-a-fourth-slot", "into-slot-0"])
@pytest.mark.parametrize("w", WEIGHTS, ids=["quarter-zero-three-quarters", "thirds"])
@pytest.mark.parametrize("which", ["dominant", "arrow", str(CB_SPAN), str(CB_SPAN + 1), str(CB_SPAN + 2)])
def test_the_combined_slot_has_the_bits_of_set_values_of_the_fold(oracle, which, w, dst):
    n, (p, i, v), nxt, d, sigma, precond = _system(oracle, which)
    values = SR.slot_values(v, seed=1)
    X, B = _start(n, 3, 31), _start(n, 3, 32)
    with _operator(n, p, i, v, nxt=nxt) as D:
        D.set_slots(4)  # the fourth: a copy of slot 0
        w4 = np.array(w + (0.0,))
        before = []
        for s in range(4):
            D.select(s)
            before.append(_reads(D, X, B, d, sigma, precond)[:2])
        D.select(1)
        D.combine_slots(w4, dst)
        assert D.slots == (4, 1)
        want = PC.combine_ref(values + [values[0]], w4)
        D.select(dst)
        got = _reads(D, X, B, d, sigma, precond)
        with _fresh(n, p, i, want, nxt) as E:
            ref = _reads(E, X, B, d, sigma, precond)
        for a, b, what in zip(got, ref, ("A·X", "Aᵀ·X", "solve", "iterations", "relres", "adjoint solve", "its iterations", "its relres")):
            _same_bits(a, b, (which, w, dst, what))
        for s in range(4):
            if s != dst:
                D.select(s)
                for a, b in zip(_reads(D, X, B, d, sigma, precond)[:2], before[s]):
                    _same_bits(a, b, (which, w, dst, "slot", s, "keeps its bits"))
        # a second time on the result: dst = 0 now folds the slot that was just written
        D.combine_slots(w4, dst)
        vals2 = values + [values[0]]
        vals2[dst] = want
        D.select(dst)
        with _fresh(n, p, i, PC.combine_ref(vals2, w4), nxt) as E:
            for a, b in zip(_reads(D, X, B, d, sigma, precond)[:2], _reads(E, X, B, d, sigma, precond)[:2]):
                _same_bits(a, b, (which, w, dst, "combined again"))


@pytest.mark.parametrize("nslots", [16, 17])
def test_sixteen_slots_travel_as_arguments_and_seventeen_from_the_table(oracle, nslots):
    """Every slot with a weight of its own (no zero: nslots terms), into the last slot, a source; then with every second weight zero (eight or
    nine terms: the argument path on both operators)."""
    import otmb_amd.api as api

    n, (p, i, v), nxt, d, sigma, precond = _system(oracle, "dominant")
    rng = np.random.default_rng(50 + nslots)
    values = [v * rng.uniform(0.9, 1.1, v.size) for _ in range(nslots)]
    X, B = _start(n, 2, 33), _start(n, 2, 34)
    for w in (rng.uniform(0.01, 0.2, nslots), np.where(np.arange(nslots) % 2 == 0, 1.0 / nslots, 0.0)):
        with api.DeviceOperator(_csc(n, p, i, v)) as D:
            D.set_lines(nxt)
            D.set_slots(nslots)
            for s in range(nslots):
                D.set_values(values[s], slot=s)
            D.combine_slots(w, nslots - 1)
            D.select(nslots - 1)
            got = _reads(D, X, B, d, sigma, precond)
            D.select(0)
            first = _reads(D, X, B, d, sigma, precond)[:2]
        with _fresh(n, p, i, PC.combine_ref(values, w), nxt) as E:
            for a, b in zip(got, _reads(E, X, B, d, sigma, precond)):
                _same_bits(a, b, (nslots, "combined"))
        with _fresh(n, p, i, values[0], nxt) as E:
            for a, b in zip(first, _reads(E, X, B, d, sigma, precond)[:2]):
                _same_bits(a, b, (nslots, "slot 0 keeps its bits"))


def test_all_weights_zero_give_plus_zero(oracle):
    n, (p, i, v), nxt, d, sigma, precond = _system(oracle, str(CB_SPAN + 1))
    X = _start(n, 2, 35)
    with _operator(n, p, i, v, nxt=nxt) as D:
        D.combine_slots([0.0, 0.0, 0.0], 2)
        D.select(2)
        for adjoint in (False, True):
            Y = D.mul(X, adjoint=adjoint)
            assert not Y.any() and not np.signbit(Y).any()


def test_refusals_write_nothing_and_leave_the_operator_usable(oracle):
    from otmb_amd import capi

    n, (p, i, v), nxt, d, sigma, precond = _system(oracle, "dominant")
    X, B = _start(n, 2, 36), _start(n, 2, 37)
    with _operator(n, p, i, v, nxt=nxt) as D:
        before = []
        for s in range(3):
            D.select(s)
            before.append(_reads(D, X, B, d, sigma, precond))
        D.select(2)
        for w, dst in (((1.0, np.nan, 0.0), 0), ((np.inf, 0.0, 0.0), 1), ((0.0, 0.0, -np.inf), 2), ((0.5, 0.5, 0.0), 3), ((0.5, 0.5, 0.0), -1)):
            with pytest.raises(capi.OtmbError) as e:
                D.combine_slots(w, dst)
            assert e.value.name == "INVALID_ARG" and "combine_slots" in str(e.value), (w, dst, str(e.value))
            assert D.slots == (3, 2)
        with pytest.raises(capi.OtmbError):
            D.combine_slots((0.5, 0.5), 0)  # one weight per slot
        w = np.array([0.5, 0.5, 0.0])
        assert capi.lib().otmb_op_combine_slots(D.handle, None, 0) == 11
        assert capi.lib().otmb_op_combine_slots_dev(D.handle, w.ctypes.data, 3) == 11
        for s in range(3):
            D.select(s)
            for a, b in zip(_reads(D, X, B, d, sigma, precond), before[s]):
                _same_bits(a, b, ("after the refusals, slot", s))
        D.combine_slots(w, 2)  # and it is usable
        D.select(2)
        with _fresh(n, p, i, PC.combine_ref(SR.slot_values(v, seed=1), w), nxt) as E:
            for a, b in zip(_reads(D, X, B, d, sigma, precond), _reads(E, X, B, d, sigma, precond)):
                _same_bits(a, b, "after the refusals")


def test_the_device_operator_and_the_assemblers_bookkeeping():
    """device.Operator.combine_slots (otmb_op_combine_slots_dev on torch's stream) through DeviceAssembler.combine_slots on three kept months:
    the mean of the months in a fourth slot has the bits of api.DeviceOperator's; written over the selected slot, the operator no longer
    holds the resident result there, so operator() raises until keep_slot() says where the result goes."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _fields, _host, _pair

    g, gm, asm, other, umo, vmo, fill = _pair("small_rho3d")
    del other
    N = asm.N
    fields = _fields(umo, vmo, 3, seed=5)
    months = []
    for m in range(3):
        asm.step(*fields[m], fill)
        asm.keep_slot(m, nslots=4)
        months.append(_host(asm)["T"])
    w = np.array([1 / 3, 1 / 3, 1 / 3, 0.0])
    X = _start(N, 2, 38)
    Xd = torch.from_numpy(X).cuda().t().contiguous().t()
    op = asm.combine_slots(w, 3)
    assert op.slots == (4, 2)
    op.select(3)
    got = [op.mul(Xd).cpu().numpy(), op.mul(Xd, adjoint=True).cpu().numpy()]
    op.select(2)
    assert asm.operator("T") is op  # slot 2 still holds the resident result
    p, i, _ = months[0]
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, PC.combine_ref([m[2] for m in months], w[:3]))) as E:
        _same_bits(got[0], E.mul(X), "the mean of the months, A·X")
        _same_bits(got[1], E.mul(X, adjoint=True), "the mean of the months, Aᵀ·X")
    asm.combine_slots(w, 2)  # over the selected slot
    with pytest.raises(ValueError, match="keep_slot"):
        asm.operator("T")
    asm.keep_slot(2)
    assert asm.operator("T") is op
    _same_bits(op.mul(Xd).cpu().numpy(), api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, months[2][2])).mul(X), "keep_slot puts the result back")
    with pytest.raises(ValueError, match="keep_slot"):
        asm.combine_slots(w, 0, matrix="Tadv")
