"""GPU: otmb_op_add_matrix (csrc/otmb_addmat.hip): slot = slot + α·B in place on a resident operator, for a B whose pattern lies inside the
operator's.  After the call to_csc(slot) is the numpy restatement by positions (tests/sink_ref.py: add_matrix_ref) bit for bit for the written
slots and untouched for the others, and A·X and Aᵀ·X have THE BITS of a fresh operator made from the restated sum -- the row layout received
the same values as the CSC copy.  Every refusal leaves every slot as it was.

Operators: tiny_tripolar's T with the three slots of tests/step_ref.py and S = the settling operator of tests/sink_ref.py; solve_ref.arrow(600)
-- a long row, so `dst` points behind the slices -- stored with one column's rows reversed and a duplicated row, and B's that name the
duplicated position, with and without duplicates of their own (the two update kernels); B with the operator's whole pattern; an empty B; B
inside padded device arrays through the `_dev` export; 8, 9 and 12 slots in one call (AM_ARGS = 8 slots' pointers travel as arguments: the
last count on that path, the first from the device table, and a year).  End to end on tiny_tripolar with three kept months:
asm.add_matrix(asm.sinking(w)) then step_tracers(d = r, precond = "lines") has the bits of an operator whose slots were set from the
host-summed values; DeviceOperator(S).solve(ones, d = r, precond = "lines") takes the restatement's one iteration."""
import numpy as np
import pytest

import sink_ref as K
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from helpers import make_case
from test_step import _csc, _operator, _same_bits, _start

pytestmark = pytest.mark.gpu

W = 1.0e-3
RATE = 1.0 / (100 * R.DAY)
RTOL, MAXITER = 1e-10, 5000
AM_ARGS = 8  # csrc/otmb_addmat.hip

_MEMO = {}


def _tiny(oracle, name="tiny_tripolar"):
    """(N, T's arrays, next, S's arrays) of a helpers grid: S with a speed per cell, NaN on land."""
    if name not in _MEMO:
        T, N, nsurf, nxt = LR.grid(oracle, name)
        g, gm = make_case(name)
        v3D, area = np.asarray(gm.v3D), np.asarray(gm.area2D)
        w = np.where(np.isnan(v3D), np.nan, np.random.default_rng(2).uniform(0.2, 2.0, v3D.shape) * W)
        _MEMO[name] = (N, T, nxt, K.sink_ref(w, v3D, area))
    return _MEMO[name]


def _fresh(n, p, i, values, nxt=None):
    import otmb_amd.api as api

    E = api.DeviceOperator(_csc(n, p, i, values))
    if nxt is not None:
        E.set_lines(nxt)
    return E


def _slots_of(D):
    return [D.to_csc(s) for s in range(D.slots[0])]


def _check(D, n, p, i, want, X, what, products=None):
    """Every slot of D: the pattern as created, nzval the bits of want[s]; A·X and Aᵀ·X of the slots in `products` (None: all) those of a fresh
    operator made from want[s]."""
    selected = D.slots[1]
    for s, w in enumerate(want):
        A = D.to_csc(s)
        assert np.array_equal(A.colptr, p) and np.array_equal(A.rowval, i), (what, s, "pattern")
        _same_bits(A.nzval, w, (what, "slot", s, "nzval"))
    for s in (range(len(want)) if products is None else products):
        D.select(s)
        with _fresh(n, p, i, want[s]) as E:
            _same_bits(D.mul(X), E.mul(X), (what, "slot", s, "A·X"))
            _same_bits(D.mul(X, adjoint=True), E.mul(X, adjoint=True), (what, "slot", s, "Aᵀ·X"))
    D.select(selected)


@pytest.mark.parametrize("slots", [None, 1, [2, 0]], ids=["every-slot", "slot-1", "slots-2-0"])
@pytest.mark.parametrize("alpha", [1.0, -0.5, 0.0])
def test_the_written_slots_are_the_restatement_and_the_others_untouched(oracle, alpha, slots):
    N, (p, i, v), nxt, S = _tiny(oracle)
    values = SR.slot_values(v, seed=1)
    want = K.add_matrix_ref(p, i, values, S, alpha, slots)
    written = range(3) if slots is None else np.atleast_1d(slots)
    for s in range(3):  # (the restatement itself: the other slots are the arrays given, a zero α writes nothing)
        assert np.array_equal(want[s], values[s]) == (s not in written or alpha == 0.0)
    X = _start(N, 3, 41)
    with _operator(N, p, i, v, nxt=nxt) as D:
        D.select(1)
        D.add_matrix(_csc(N, *S), alpha=alpha, slots=slots)
        assert D.slots == (3, 1)
        _check(D, N, p, i, want, X, (alpha, slots))
        if alpha == 1.0 and slots is None:  # a second time, on the result
            D.add_matrix(_csc(N, *S), alpha=0.25)
            _check(D, N, p, i, K.add_matrix_ref(p, i, want, S, 0.25), X, "twice")


def _corner(N, p, i):
    """T's pattern and one entry more: (row N, column 1), which T does not store; -> (B's arrays, the entry's 0-based position)."""
    assert N not in i[p[0] - 1 : p[1] - 1]
    e = int(p[1] - 1)  # behind column 1's entries: rows stay ascending
    Bp = p.copy()
    Bp[1:] += 1
    return (Bp, np.insert(i, e, N), np.ones(len(i) + 1)), e


def test_an_entry_outside_the_pattern_is_named_and_nothing_is_written(oracle):
    from otmb_amd import capi

    N, (p, i, v), nxt, S = _tiny(oracle)
    B, e = _corner(N, p, i)
    with pytest.raises(K.PatternNotContained) as ref:
        K.add_matrix_ref(p, i, SR.slot_values(v, seed=1), B)
    assert (ref.value.entry, ref.value.row, ref.value.col) == (e, N, 1)
    X = _start(N, 2, 42)
    with _operator(N, p, i, v, nxt=nxt) as D:
        for alpha, slots in ((1.0, None), (0.0, None), (2.0, [1])):
            with pytest.raises(capi.OtmbError) as err:
                D.add_matrix(_csc(N, *B), alpha=alpha, slots=slots)
            assert err.value.status == 21 and err.value.name == "PATTERN_NOT_CONTAINED"
            assert str(ref.value) in str(err.value), str(err.value)
        # two misses: the first in B's stored order is the one named
        B2 = (B[0].copy(), B[1].copy(), B[2])
        last = int(B2[0][N - 1] - 1)  # the first entry of the last column: make it row 1, which that column does not store
        assert 1 not in i[p[N - 1] - 1 : p[N] - 1]
        B2[1][last] = 1
        with pytest.raises(capi.OtmbError) as err:
            D.add_matrix(_csc(N, *B2))
        assert str(ref.value) in str(err.value)
        _check(D, N, p, i, SR.slot_values(v, seed=1), X, "after the misses")
        D.add_matrix(_csc(N, *S))  # and it is usable
        _check(D, N, p, i, K.add_matrix_ref(p, i, SR.slot_values(v, seed=1), S), X, "after the refusals", products=[0])


def test_bad_indices_slots_and_shapes_are_invalid_arguments(oracle):
    import otmb_amd.api as api
    from otmb_amd import capi

    N, (p, i, v), nxt, (Sp, Si, Sx) = _tiny(oracle)
    X = _start(N, 2, 43)
    with _operator(N, p, i, v, nxt=nxt) as D:
        bad = []
        for r in (0, N + 1, -3):
            Bi = Si.copy()
            Bi[5] = r
            bad.append(((Sp, Bi, Sx), {}))
        Bp = Sp.copy()
        c = int(np.flatnonzero(np.diff(Sp) == 2)[3])
        Bp[c + 1] = Bp[c] - 1  # not monotone, the two ends as they were
        bad.append(((Bp, Si, Sx), {}))
        Bp = Sp.copy()
        Bp[N // 2] = len(Si) + 5  # beyond nnz + 1
        bad.append(((Bp, Si, Sx), {}))
        bad.append(((Sp + 1, Si, Sx), {}))  # colptr[1] != 1
        for kw in (dict(slots=3), dict(slots=-1), dict(slots=[0, 0]), dict(slots=[0, 1, 2, 1]), dict(alpha=np.nan), dict(alpha=np.inf)):
            bad.append(((Sp, Si, Sx), kw))
        for B, kw in bad:
            with pytest.raises(capi.OtmbError) as err:
                D.add_matrix(api.SparseMatrixCSC(N, N, *B), **kw)
            assert err.value.name == "INVALID_ARG", (kw, str(err.value))
        with pytest.raises(capi.OtmbError) as err:  # another shape
            D.add_matrix(api.SparseMatrixCSC(N + 1, N + 1, np.append(Sp, Sp[-1]), Si, Sx))
        assert err.value.name == "INVALID_ARG"
        lib = capi.lib()
        assert lib.otmb_op_add_matrix(D.handle, N, N, None, Si.ctypes.data, Sx.ctypes.data, 1.0, 0, None) == 11
        assert lib.otmb_op_add_matrix(D.handle, N, N + 1, Sp.ctypes.data, Si.ctypes.data, Sx.ctypes.data, 1.0, 0, None) == 11
        assert lib.otmb_op_add_matrix(None, N, N, Sp.ctypes.data, Si.ctypes.data, Sx.ctypes.data, 1.0, 0, None) == 11
        _check(D, N, p, i, SR.slot_values(v, seed=1), X, "after the refusals", products=[0, 2])
        D.add_matrix(api.SparseMatrixCSC(N, N, Sp, Si, Sx), slots=[])  # no slot: checked, nothing written
        _check(D, N, p, i, SR.slot_values(v, seed=1), X, "no slot requested", products=[])


def _shuffled_arrow():
    """solve_ref.arrow(600) stored with column 1's rows reversed and row 1 stored twice in column 6 (1-based): (colptr, rowval, nzval)."""
    p, i, v = R.arrow(600)
    assert np.bincount(i - 1, minlength=600).max() > 512  # row 1: a long row, behind the slices
    i, v = i.copy(), v.copy()
    a, b = p[0] - 1, p[1] - 1
    i[a:b], v[a:b] = i[a:b][::-1].copy(), v[a:b][::-1].copy()
    e = int(p[6] - 1)  # the end of column 6, whose rows are (1, 6)
    assert i[p[5] - 1 : e].tolist() == [1, 6]
    p2 = p.copy()
    p2[6:] += 1
    return p2, np.insert(i, e, 1), np.insert(v, e, 0.375)


@pytest.mark.parametrize("duplicates", [False, True], ids=["distinct-B", "B-names-a-position-twice"])
def test_the_first_stored_match_receives_the_value(duplicates):
    """Unsorted and duplicate rows in the operator, a long row, and a B that names the duplicated position -- with B's own duplicates the
    additions into one position happen in B's stored order (the column kernel)."""
    import otmb_amd.api as api

    n = 600
    p, i, v = _shuffled_arrow()
    first = int(p[5] - 1)  # column 6 stores rows (1, 6, 1): (1, 6) is matched at `first`, never at the third entry
    assert i[first : first + 3].tolist() == [1, 6, 1]
    rng = np.random.default_rng(44)
    cols, rows = [], []
    rows0 = [600, 3, 1, 77, 512, 513] + ([3, 600, 3] if duplicates else [])  # column 1 (stored reversed), in an order of B's own
    cols += [1] * len(rows0)
    rows += rows0
    cols += [6] * (3 if duplicates else 2)
    rows += [6, 1] + ([1] if duplicates else [])
    for c in (2, 300, 600):  # the long row and the diagonal elsewhere
        cols += [c, c]
        rows += [c, 1]
    order = np.argsort(np.array(cols), kind="stable")
    cols, rows = np.array(cols)[order], np.array(rows)[order]
    Bp = np.concatenate(([1], 1 + np.cumsum(np.bincount(cols - 1, minlength=n)))).astype(np.int64)
    B = (Bp, rows.astype(np.int64), rng.uniform(0.5, 1.5, len(rows)))
    values = SR.slot_values(v, seed=3)
    want = K.add_matrix_ref(p, i, values, B, -1.75)
    pos = K.match_positions(p, i, B[0], B[1])
    assert first in pos and first + 2 not in pos and (len(set(pos)) < len(pos)) == duplicates
    _same_bits(want[0][first + 2], values[0][first + 2], "the later duplicate is never written")
    X = _start(n, 2, 45)
    with api.DeviceOperator(_csc(n, p, i, v)) as D:
        D.set_slots(3)
        for s in range(3):
            D.set_values(values[s], slot=s)
        D.add_matrix(_csc(n, *B), alpha=-1.75)
        _check(D, n, p, i, want, X, ("arrow", duplicates))


def test_the_whole_pattern_and_an_empty_matrix(oracle):
    N, (p, i, v), nxt, S = _tiny(oracle)
    values = SR.slot_values(v, seed=1)
    X = _start(N, 2, 46)
    full = (p, i, np.random.default_rng(47).standard_normal(len(v)) * np.abs(v))
    empty = (np.ones(N + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
    with _operator(N, p, i, v, nxt=nxt) as D:
        D.add_matrix(_csc(N, *empty), alpha=3.0)
        _check(D, N, p, i, values, X, "empty", products=[1])
        D.add_matrix(_csc(N, *full), alpha=0.75, slots=[0, 2])
        want = K.add_matrix_ref(p, i, values, full, 0.75, [0, 2])
        _same_bits(want[0], values[0] + 0.75 * full[2], "the whole pattern is an elementwise sum")
        _check(D, N, p, i, want, X, "the whole pattern")


@pytest.mark.parametrize("name,nslots", [("tiny_tripolar", AM_ARGS), ("tiny_tripolar", AM_ARGS + 1), ("small_rho3d", 12)])
def test_eight_slots_travel_as_arguments_nine_and_a_year_from_the_table(oracle, name, nslots):
    import otmb_amd.api as api

    N, (p, i, v), nxt, S = _tiny(oracle, name)
    rng = np.random.default_rng(60 + nslots)
    values = [v * rng.uniform(0.9, 1.1, v.size) for _ in range(nslots)]
    X = _start(N, 2, 48)
    with api.DeviceOperator(_csc(N, p, i, v)) as D:
        D.set_slots(nslots)
        for s in range(nslots):
            D.set_values(values[s], slot=s)
        D.add_matrix(_csc(N, *S), alpha=1.0)
        want = K.add_matrix_ref(p, i, values, S, 1.0)
        _check(D, N, p, i, want, X, (name, nslots), products=[0, nslots - 1])
        if nslots > AM_ARGS:  # and a list longer than the argument path, in an order of its own
            sel = list(range(nslots - 1, -1, -1))[: AM_ARGS + 1]
            D.add_matrix(_csc(N, *S), alpha=-1.0, slots=sel)
            _check(D, N, p, i, K.add_matrix_ref(p, i, want, S, -1.0, sel), X, (name, nslots, "a list"), products=[sel[0]])


def test_the_dev_entry_on_padded_device_arrays(oracle):
    """otmb_op_add_matrix_dev with B's three arrays INSIDE larger device buffers -- a pad in front (so no array starts an allocation) and
    behind, holding sentinels that would be out of range as indices: the inputs keep their bits, padding included, and the slots are the
    restatement's; a miss through this entry leaves the slots alone too."""
    import torch

    from otmb_amd.device import DeviceAssembler, Operator

    N, (p, i, v), nxt, (Sp, Si, Sx) = _tiny(oracle)
    ctx = DeviceAssembler(0).ctx  # (on torch's current stream)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    O = Operator(ctx, N, N, t(p, np.int64), t(i, np.int64), t(v, np.float64))
    O.set_slots(3)
    values = SR.slot_values(v, seed=1)
    for s in range(3):
        O.set_values_dev(t(values[s], np.float64), slot=s)

    def padded(a, front, back, fill):
        buf = torch.full((front + len(a) + back,), fill, dtype=torch.from_numpy(a).dtype, device="cuda")
        buf[front : front + len(a)] = torch.from_numpy(a).cuda()
        return buf, buf[front : front + len(a)]

    def slots_now():
        torch.cuda.synchronize()
        return [O.to_csc(s)[2].cpu().numpy() for s in range(3)]

    bufs = [padded(Sp, 3, 5, -(2 ** 40)), padded(Si, 1, 7, 2 ** 40), padded(Sx, 5, 3, np.nan)]
    before = [b.clone() for b, _ in bufs]
    sel = np.array([2, 0], dtype=np.int64)
    rc = O.lib.otmb_op_add_matrix_dev(O.handle, N, N, bufs[0][1].data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), 0.5, 2, sel.ctypes.data)
    assert rc == 0, ctx._lib.otmb_last_error(ctx.handle)
    want = K.add_matrix_ref(p, i, values, (Sp, Si, Sx), 0.5, [2, 0])
    for s, got in enumerate(slots_now()):
        _same_bits(got, want[s], ("padded", "slot", s))
    for (b, _), was in zip(bufs, before):
        assert torch.equal(b.view(torch.int64), was.view(torch.int64)), "an input changed"
    # through the tensors' binding, and the row layout through a product
    O.add_matrix(tuple(view for _, view in bufs), alpha=-2.0, slots=1)
    want = K.add_matrix_ref(p, i, want, (Sp, Si, Sx), -2.0, 1)
    X = _start(N, 2, 49)
    O.select(1)
    with _fresh(N, p, i, want[1]) as E:
        Xd = torch.from_numpy(X).cuda().t().contiguous().t()
        _same_bits(O.mul(Xd).cpu().numpy(), E.mul(X), "A·X after the tensors' binding")
        _same_bits(O.mul(Xd, adjoint=True).cpu().numpy(), E.mul(X, adjoint=True), "Aᵀ·X after the tensors' binding")
    # a miss
    B, e = _corner(N, p, i)
    Bd = (t(B[0], np.int64), t(B[1], np.int64), t(B[2], np.float64))
    rc = O.lib.otmb_op_add_matrix_dev(O.handle, N, N, Bd[0].data_ptr(), Bd[1].data_ptr(), Bd[2].data_ptr(), 1.0, 0, None)
    assert rc == 21 and f"entry {e + 1} of B, (row {N}, column 1)" in ctx._lib.otmb_last_error(ctx.handle).decode()
    for s, got in enumerate(slots_now()):
        _same_bits(got, want[s], ("after the miss", "slot", s))
    O.close()


def test_end_to_end_sinking_added_to_three_kept_months_then_stepped():
    """asm.add_matrix(asm.sinking(w)) on three kept months, then step_tracers(d = r, precond = "lines"): the bits of the same call on an
    operator whose slots were set from the host-summed values; and the assembler's bookkeeping is combine_slots'."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _fields, _host, _pair

    g, gm, asm, other, umo, vmo, fill = _pair("tiny_tripolar")
    del other
    N = asm.N
    v3D, area = np.asarray(gm.v3D), np.asarray(gm.area2D)
    w = np.asfortranarray(np.where(np.isnan(v3D), np.nan, np.random.default_rng(2).uniform(0.2, 2.0, v3D.shape) * W))
    months = []
    for m, (u, v) in enumerate(_fields(umo, vmo, 3, seed=6)):
        asm.step(u, v, fill)
        asm.keep_slot(m, nslots=3)
        months.append(_host(asm)["T"])
    p, i, _ = months[0]
    assert all(np.array_equal(mm[0], p) and np.array_equal(mm[1], i) for mm in months)
    S = asm.sinking(w)
    Sh = tuple(x.cpu().numpy() for x in S)
    assert all(np.array_equal(a, b) for a, b in zip(Sh[:2], K.sink_ref(w, v3D, area)[:2]))
    _same_bits(Sh[2], K.sink_ref(w, v3D, area)[2], "S")
    op = asm.add_matrix(S)
    assert op.slots == (3, 2)
    with pytest.raises(ValueError, match="keep_slot"):  # the selected slot no longer holds the resident result
        asm.operator("T")
    summed = K.add_matrix_ref(p, i, [mm[2] for mm in months], Sh)
    X = _start(N, 2, 50)
    Xd = torch.from_numpy(X).cuda().t().contiguous().t()
    r = np.full(N, RATE)
    kw = dict(dt=SR.MONTH, theta=1.0, nsteps=6, first_slot=1, rtol=RTOL, maxiter=MAXITER, precond="lines")
    got, ginfo = asm.step_tracers(Xd, d=torch.from_numpy(r).cuda(), **kw)
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, summed[0])) as E:
        E.set_lines(api.vertical_lines(dict(Lwet3D=asm.lwet3d.cpu().numpy().reshape(v3D.shape, order="F"), N=N)))
        E.set_slots(3)
        for s in range(3):
            E.set_values(summed[s], slot=s)
        ref, rinfo = E.step(X, d=r, **kw)
    assert ginfo.steps_done == rinfo.steps_done == 6 and np.array_equal(ginfo.iterations, rinfo.iterations)
    _same_bits(got.cpu().numpy(), ref, "six steps through T + S")
    print("iterations per step", ginfo.iterations.tolist())
    # a slot that is not the selected one leaves the record clean
    asm.keep_slot(2)
    asm.add_matrix(S, alpha=0.5, slots=[0, 1])
    assert asm.operator("T") is op
    with pytest.raises(ValueError, match="keep_slot"):
        asm.add_matrix(S, matrix="Tadv")


def test_the_settling_operator_alone_solves_in_the_restatements_one_iteration(oracle):
    import otmb_amd.api as api

    N, T, nxt, S = _tiny(oracle)
    A = R.csc_of(N, N, *S)
    ones, r = np.ones(N), np.full(N, RATE)
    _, rinfo = LR.solve_lines_ref(A, ones, nxt, d=r, rtol=RTOL)
    assert rinfo["iterations"].tolist() == [1]
    with api.DeviceOperator(_csc(N, *S)) as D:
        D.set_lines(nxt)
        X, info = D.solve(ones, d=r, rtol=RTOL, maxiter=MAXITER, precond="lines")
    assert info.converged.all() and info.iterations.tolist() == rinfo["iterations"].tolist() == [1], info
    (res, bound), = R.residual_check(A, X, ones, r, 0.0, False, RTOL)
    print("residual", res, "bound", bound)
    assert res <= bound
