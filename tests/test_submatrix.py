"""otmb_op_submatrix / otmb_op_take_values / otmb_op_fetch / otmb_op_get_lines on the device (csrc/otmb_submatrix.hip; include/otmb.h): the child of
a submatrix call is INDISTINGUISHABLE from its twin -- the operator otmb_op_create makes from the restated A[rows, cols] (tests/submatrix_ref.py),
with its slots set from the restated values and its lines from the restated next.  Equal means equal in bits: the matrix each reports, the
lines, the slots, the products, and on diagonally dominant systems the solver's every answer and a stepped state."""
import numpy as np
import pytest

import solve_lines_ref as LR
import solve_ref as R
import spmv_edges as E
import step_ref as SR
import submatrix_ref as SUB
from spmv_ref import bits, random_dense

pytestmark = pytest.mark.gpu

INVALID_ARG = 11


def _api():
    import otmb_amd.api as api

    return api


def _parent(m, n, p, i, v, nxt=None, select=0):
    """(the parent with the three slots of step_ref.slot_values and, where given, lines; the slots' values)."""
    api = _api()
    nnz = int(p[-1] - 1)
    p, i, v = np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64)[:nnz], np.asarray(v, dtype=np.float64)[:nnz]
    vals = SR.slot_values(v, seed=1)
    D = api.DeviceOperator(api.SparseMatrixCSC(m, n, p, i, vals[0]))
    D.set_slots(3)
    for s in (1, 2):
        D.set_values(vals[s], slot=s)
    if nxt is not None:
        D.set_lines(nxt)
    D.select(select)
    return D, vals


def _twin(m, n, p, i, vals, nxt, rows, cols, select=0):
    """The operator otmb_op_create makes from the restatement's arrays; (it, the gather table)."""
    api = _api()
    cpc, rvc, src = SUB.submatrix_ref(m, n, p, i, rows, cols)
    T = api.DeviceOperator(api.SparseMatrixCSC(len(rows), len(cols), cpc, rvc, vals[0][src]))
    T.set_slots(len(vals))
    for s in range(1, len(vals)):
        T.set_values(vals[s][src], slot=s)
    if nxt is not None and len(rows) == len(cols) and np.array_equal(rows, cols):
        T.set_lines(SUB.restrict_lines(nxt, rows))
    T.select(select)
    return T, src


def _same_matrix(C, T, what):
    assert C.shape == T.shape and C.nnz == T.nnz and C.slots == T.slots, what
    lc, lt = C.lines, T.lines
    assert (lc is None) == (lt is None) and (lc is None or np.array_equal(lc, lt)), (what, "lines")
    for s in range(C.slots[0]):
        a, b = C.to_csc(s), T.to_csc(s)
        assert np.array_equal(a.colptr, b.colptr) and np.array_equal(a.rowval, b.rowval), (what, s)
        assert np.array_equal(a.nzval.view(np.int64), b.nzval.view(np.int64)), (what, s, "nzval bits")
    a, b = C.to_csc(), T.to_csc()  # the selected slot
    assert np.array_equal(a.nzval.view(np.int64), b.nzval.view(np.int64)), (what, "selected")


def _same_products(C, T, what, ks=(1, 3, 8), seed=3):
    m, n = C.shape
    if m == 0 or n == 0:
        return
    rng = np.random.default_rng(seed)
    for k in ks:
        X, Y = random_dense(rng, n, k, specials=False), random_dense(rng, m, k, specials=False)
        assert np.array_equal(bits(C.mul(X)), bits(T.mul(X))), (what, k)
        assert np.array_equal(bits(C.mul(Y, adjoint=True)), bits(T.mul(Y, adjoint=True))), (what, k, "adjoint")


def _same_report(ic, it, keys, what):
    assert ic.status == it.status, what
    for key in keys:
        a, b = getattr(ic, key), getattr(it, key)
        if key == "reason":
            assert a == b, (what, key)
        elif np.asarray(a).dtype.kind == "f":
            assert np.array_equal(bits(a), bits(b)), (what, key)
        else:
            assert np.array_equal(a, b), (what, key)


def _same_solves(C, T, what, dt):
    """solve with both preconditioners (lines where the pair has them) and one step call of 4 steps over the 3 slots, θ = 0.5."""
    n = C.shape[0]
    rng = np.random.default_rng(7)
    B = np.asfortranarray(rng.standard_normal((n, 3)))
    for pc in ("jacobi",) + (("lines",) if C.lines is not None else ()):
        Xc, ic = C.solve(B, precond=pc, rtol=1e-10, maxiter=500)
        Xt, it = T.solve(B, precond=pc, rtol=1e-10, maxiter=500)
        assert ic.converged.all(), (what, pc, ic)
        assert np.array_equal(bits(Xc), bits(Xt)), (what, pc)
        _same_report(ic, it, ("iterations", "relres", "reason"), (what, pc))
        kw = dict(dt=dt, theta=0.5, nsteps=4, first_slot=0, precond=pc, rtol=1e-10, maxiter=500)
        Xc, ic = C.step(B, **kw)
        Xt, it = T.step(B, **kw)
        assert ic.steps_done == it.steps_done == 4, (what, pc, ic)
        assert np.array_equal(bits(Xc), bits(Xt)), (what, pc, "step")
        _same_report(ic, it, ("iterations", "relres", "reason"), (what, pc, "step"))


def _check(P, fx, vals, nxt, rows, cols, what, products=True, solves=None, select=0):
    m, n, p, i = fx
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    principal = len(rows) == len(cols) and np.array_equal(rows, cols)
    C = P.submatrix(rows) if principal else P.submatrix(rows, cols)
    T, src = _twin(m, n, p, i, vals, nxt, rows, cols, select=select)
    try:
        _same_matrix(C, T, what)
        if products:
            _same_products(C, T, what)
        if solves is not None:
            _same_solves(C, T, what, solves)
    finally:
        C.close()
        T.close()


def _half(rng, limit):
    return np.sort(rng.choice(limit, size=limit // 2, replace=False)).astype(np.int64)


# ---- the threshold fixtures ----------------------------------------------------------------------------------------------------------------
def _signature(m, n, colptr, rowval):
    """What spmv_edges' thresholds read of a layout: long rows and their chunks, the widest slice, slices, the last slice's rows, row
    workgroups, Aᵀ waves, their runs and the columns across a chunk edge."""
    L = E.layout(m, n, colptr, rowval)
    return (int(L.long.sum()), tuple(sorted(E.long_chunks(int(x)) for x in L.lens[L.long])), int(L.width.max()) if L.nslices else 0, L.nslices,
            int(L.slice_rows[-1]) if L.nslices else 0, L.row_wgs, L.waves, tuple(int(r) for r in L.run), tuple(sorted((c, tuple(o)) for c, o in L.cross.items())))


def _focus_drop(f):
    """(rows, cols) that drop exactly the fixture's focus: its long (or at-threshold) row, its focus columns, or -- the size fixtures, whose
    thresholds are counts -- the last row and the last column."""
    rows, cols = np.arange(f.m), np.arange(f.n)
    if f.name.startswith("size_"):
        return rows[:-1], cols[:-1]
    if f.name.startswith(("run", "cols_")):
        drop = np.asarray(getattr(f, "straddlers", f.focus["cols"]), dtype=np.int64)
        return rows, np.delete(cols, drop)
    drop = f.focus["long"] if "long" in f.focus else f.focus["rows"]
    assert len(drop) == 1
    return np.delete(rows, drop), cols


@pytest.mark.parametrize("name", E.THRESHOLD_FIXTURES)
def test_threshold_fixtures_under_three_selections(name):
    f = E.fixtures()[name]
    fx = (f.m, f.n, np.asarray(f.colptr, dtype=np.int64), np.asarray(f.rowval, dtype=np.int64))
    nxt = LR.random_lines(f.n, 5) if f.m == f.n else None
    P, vals = _parent(f.m, f.n, f.colptr, f.rowval, f.nzval, nxt=nxt, select=2)
    rng = np.random.default_rng(17)
    try:
        _check(P, fx, vals, nxt, np.arange(f.m), np.arange(f.n), (name, "all"), select=2)
        _check(P, fx, vals, nxt, _half(rng, f.m), _half(rng, f.n), (name, "half"), select=2)
        rows, cols = _focus_drop(f)
        cpc, rvc, _ = SUB.submatrix_ref(*fx, rows, cols)
        before, after = _signature(*fx), _signature(len(rows), len(cols), cpc, rvc)
        print(name, "layout", before[:7], "->", after[:7])
        assert before != after, (name, "the child's layout is the parent's")
        _check(P, fx, vals, nxt, rows, cols, (name, "focus dropped"), select=2)
        assert P.slots == (3, 2)
    finally:
        P.close()


def test_mixed_with_its_long_row_and_column_kept_and_thinned():
    f = E.fixtures()["mixed"]
    fx = (f.m, f.n, np.asarray(f.colptr, dtype=np.int64), np.asarray(f.rowval, dtype=np.int64))
    rng = np.random.default_rng(19)
    rows, cols = np.union1d(_half(rng, f.m), [70]), np.union1d(_half(rng, f.n), [130])
    cpc, rvc, _ = SUB.submatrix_ref(*fx, rows, cols)
    L = E.layout(len(rows), len(cols), cpc, rvc)
    r70, c130 = int(np.searchsorted(rows, 70)), int(np.searchsorted(cols, 130))
    assert L.long[r70] and 100 < L.lens[r70] < 600 and 100 < np.diff(cpc)[c130] < 800  # kept, and thinned
    nxt = LR.random_lines(f.n, 6)
    P, vals = _parent(f.m, f.n, f.colptr, f.rowval, f.nzval, nxt=nxt)
    try:
        _check(P, fx, vals, nxt, rows, cols, "mixed thinned")
        _check(P, fx, vals, nxt, rows, rows, "mixed thinned, principal")
    finally:
        P.close()


# ---- diagonally dominant systems: the solver and the step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dominant257", "arrow600"])
def test_principal_submatrices_of_dominant_systems(which):
    """256, 257, 1 and n - 1 selected: one and two workgroups of the plan kernels; arrow's first row and column (n entries each) kept and dropped."""
    n = 257 if which == "dominant257" else 600
    p, i, v = R.dominant(n) if which == "dominant257" else R.arrow(n)
    fx = (n, n, p, i)
    nxt = LR.random_lines(n, 8)
    P, vals = _parent(n, n, p, i, v, nxt=nxt)
    sels = {"first 256": np.arange(256), "257 from the second": np.arange(1, 258) if n > 257 else np.arange(257), "one": np.array([n // 2]),
            "n - 1 without the first": np.arange(1, n), "n - 1 without the last": np.arange(n - 1)}
    try:
        for what, sel in sels.items():
            _check(P, fx, vals, nxt, sel, sel, (which, what), solves=1.0)
    finally:
        P.close()


@pytest.mark.parametrize("name", ["odd_nx_fold", "tiny_tripolar"])
def test_grids_with_the_surface_and_with_random_cells_dropped(oracle, name):
    T, N, nsurf, nxt = LR.grid(oracle, name)
    p, i, v = T
    fx = (N, N, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64))
    P, vals = _parent(N, N, p, i, v, nxt=nxt)
    try:
        for what, sel in (("surface", np.arange(nsurf, N)), ("random", np.flatnonzero(np.random.default_rng(23).random(N) >= 0.3))):
            C = P.submatrix(sel)
            Tw, _ = _twin(*fx, vals, nxt, sel, sel)
            try:
                _same_matrix(C, Tw, (name, what))
                _same_products(C, Tw, (name, what))
                B = np.asfortranarray(np.random.default_rng(29).standard_normal((len(sel), 3)))
                kw = dict(dt=SR.MONTH, theta=0.5, nsteps=4, first_slot=0, precond="lines", rtol=1e-10, maxiter=2000)
                (Xc, ic), (Xt, it) = C.step(B, **kw), Tw.step(B, **kw)
                assert ic.steps_done == it.steps_done == 4, (name, what, ic)
                assert np.array_equal(bits(Xc), bits(Xt)), (name, what, "step")
                _same_report(ic, it, ("iterations", "relres", "reason"), (name, what, "step"))
            finally:
                C.close()
                Tw.close()
    finally:
        P.close()


def test_a_scan_of_many_blocks_and_more_than_one_trip(oracle):
    """90 x 60 x 20 (N = 65 817, about half a million entries), the surface dropped: to_csc and one product."""
    T, N, nsurf, nxt = LR.grid(oracle, "90x60x20")
    p, i, v = T
    fx = (N, N, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64))
    P, vals = _parent(N, N, p, i, v, nxt=nxt)
    sel = np.arange(nsurf, N)
    C = P.submatrix(sel)
    Tw, _ = _twin(*fx, vals, nxt, sel, sel)
    try:
        _same_matrix(C, Tw, "90x60x20")
        _same_products(C, Tw, "90x60x20", ks=(3,))
    finally:
        for D in (C, Tw, P):
            D.close()


# ---- take_values -------------------------------------------------------------------------------------------------------------------------------
def test_take_values_writes_one_slot_and_nothing_else():
    n = 257
    p, i, v = R.dominant(n)
    fx = (n, n, p, i)
    nxt = LR.random_lines(n, 9)
    P, vals = _parent(n, n, p, i, v, nxt=nxt, select=2)
    rng = np.random.default_rng(31)
    rows, cols = _half(rng, n), _half(rng, n)
    C = P.submatrix(rows, cols)
    Tw, src = _twin(*fx, vals, None, rows, cols, select=2)
    try:
        sentinel = np.full(C.nnz, -777.25)
        for s in range(3):
            C.set_values(sentinel, slot=s)
            Tw.set_values(sentinel, slot=s)
        new = vals[1] * rng.uniform(0.5, 2.0, len(vals[1]))
        new[::7] = -0.0
        P.set_values(new, slot=1)
        C.take_values(P, slot=1)
        Tw.set_values(new[src], slot=1)
        assert C.slots == (3, 2)
        _same_matrix(C, Tw, "after take_values")
        for s in range(3):  # both value arrays of every slot: the products read the row layout's, the adjoint ones the CSC copy's
            C.select(s)
            Tw.select(s)
            _same_products(C, Tw, ("after take_values, slot", s), ks=(3,))
        C.select(2)
        Tw.select(2)
        # another slot of the parent into another slot of the child; the default slot is the selected one
        C.take_values(P, slot=0, parent_slot=2)
        Tw.set_values(vals[2][src], slot=0)
        C.take_values(P)
        Tw.set_values(vals[2][src], slot=2)
        _same_matrix(C, Tw, "after three take_values")
        _same_products(C, Tw, "after three take_values", ks=(3,))
        # the child of a child takes from the child, which is its parent
        sub = np.arange(0, C.shape[0], 2)
        G = C.submatrix(sub, np.arange(C.shape[1]))
        G.take_values(C, slot=1)
        with pytest.raises(_api().capi.OtmbError) as e:
            G.take_values(P, slot=1)
        assert e.value.status == INVALID_ARG
        G.close()
    finally:
        for D in (C, Tw, P):
            D.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_position_and_leave_everything_usable():
    capi = _api().capi
    n = 257
    p, i, v = R.dominant(n)
    P, vals = _parent(n, n, p, i, v, nxt=LR.random_lines(n, 10))
    x = np.random.default_rng(37).standard_normal(n)
    y0 = P.mul(x)
    good = np.arange(0, n, 2)
    bad_lists = {"an index of 0": [-1, 3, 9], "an index of m + 1": [0, 5, n], "a descending pair": [2, 8, 5, 11], "a repeated index": [1, 4, 4, 9]}
    try:
        for what, lst in bad_lists.items():
            lst = np.asarray(lst, dtype=np.int64)
            pos = SUB.first_offender(lst + 1, n) + 1
            for kind, call in (("row", lambda: P.submatrix(lst, good)), ("column", lambda: P.submatrix(good, lst)), ("row", lambda: P.submatrix(lst))):
                with pytest.raises(capi.OtmbError) as e:
                    call()
                msg = str(e.value)
                print(what, "->", msg)
                assert e.value.status == INVALID_ARG and f"position {pos} " in msg and f"the {kind} index" in msg, (what, kind, msg)
                assert np.array_equal(bits(P.mul(x)), bits(y0)) and P.slots == (3, 0), what
        # take_values: another operator, an operator created after the parent was closed, slots out of range
        C = P.submatrix(good)
        Tw, _ = _twin(n, n, p, i, vals, LR.random_lines(n, 10), good, good)
        Q, _ = _parent(n, n, p, i, v)
        P2, _ = _parent(n, n, p, i, v)
        C2 = P2.submatrix(good)
        P2.close()
        P3, _ = _parent(n, n, p, i, v)  # (may lie where P2 lay: the serial number tells them apart, not the address)
        plain = _api().DeviceOperator(_api().SparseMatrixCSC(n, n, p, i, v))
        refused = {"a different operator": lambda: C.take_values(Q, slot=1), "an operator created after the parent was closed": lambda: C2.take_values(P3, slot=1),
                   "the child itself": lambda: C.take_values(C, slot=1), "an operator no submatrix call made": lambda: plain.take_values(P, slot=0),
                   "slot 3": lambda: C.take_values(P, slot=3), "slot 5": lambda: C.take_values(P, slot=1, parent_slot=5)}
        for what, call in refused.items():
            with pytest.raises(capi.OtmbError) as e:
                call()
            print(what, "->", str(e.value))
            assert e.value.status == INVALID_ARG, what
            if what.startswith("slot"):
                assert what in str(e.value)
            assert np.array_equal(bits(P.mul(x)), bits(y0)), what
        _same_matrix(C, Tw, "after the refusals")
        _same_products(C, Tw, "after the refusals", ks=(3,))
        with pytest.raises(capi.OtmbError) as e:
            C.to_csc(3)
        assert e.value.status == INVALID_ARG and "slot 3" in str(e.value)
        for D in (C, Tw, Q, C2, P3, plain):
            D.close()
    finally:
        P.close()


# ---- empty selections --------------------------------------------------------------------------------------------------------------------------
def _outcome(make):
    capi = _api().capi
    try:
        return "ok", make()
    except capi.OtmbError as e:
        return "refused", e.status


def test_empty_selections_are_what_create_makes_of_the_empty_matrix():
    """Found: otmb_op_create accepts the empty 0 x n, m x 0 and 0 x 0 matrices (nnz = 0, colptr all 1); so does otmb_op_submatrix."""
    api = _api()
    n = 64
    f = E.fixtures()["size_64x64"]
    P, vals = _parent(f.m, f.n, f.colptr, f.rowval, f.nzval, nxt=LR.random_lines(n, 11))
    none, every = np.zeros(0, dtype=np.int64), np.arange(n)
    try:
        for what, rows, cols in (("0 x n", none, every), ("m x 0", every, none), ("0 x 0", none, none)):
            empty = api.SparseMatrixCSC(len(rows), len(cols), np.ones(len(cols) + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0))
            kc, C = _outcome(lambda: P.submatrix(rows, cols))
            kt, Tw = _outcome(lambda: api.DeviceOperator(empty))
            print(what, "submatrix:", kc, "create:", kt)
            assert kc == kt, what
            if kc == "refused":
                assert C == Tw, what
                continue
            assert C.shape == Tw.shape == (len(rows), len(cols)) and C.nnz == Tw.nnz == 0 and C.slots == (3, 0), what
            a, b = C.to_csc(), Tw.to_csc()
            assert np.array_equal(a.colptr, b.colptr) and len(a.rowval) == len(b.rowval) == 0 and len(a.nzval) == len(b.nzval) == 0, what
            C.close()
            Tw.close()
        kc, C = _outcome(lambda: P.submatrix(none))  # principal and empty
        assert kc == "ok" and C.shape == (0, 0)
        C.close()
    finally:
        P.close()


# ---- fetch and get_lines on an ordinary operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["size_63x65", "size_256x256", "mixed"])
def test_fetch_returns_the_arrays_the_operator_was_created_with(name):
    """Unsorted and duplicate rows, -0.0, NaN and ±Inf: the rows as given (widened back from Int32), the values bit for bit."""
    api = _api()
    f = E.fixtures()[name]
    nnz = int(f.colptr[-1] - 1)
    p, i, v = np.asarray(f.colptr, dtype=np.int64), np.asarray(f.rowval, dtype=np.int64)[:nnz], np.asarray(f.nzval, dtype=np.float64)[:nnz].copy()
    v[:2] = np.array([0x7FF8000000ABCDEF, 0xFFF800000012345F], dtype=np.uint64).view(np.float64)  # NaNs with payloads, one negative
    assert np.isnan(v[:2]).all() and np.signbit(v).any() and (np.diff(i) < 0).any()
    with api.DeviceOperator(api.SparseMatrixCSC(f.m, f.n, p, i, v)) as D:
        assert D.lines is None
        A = D.to_csc()
        assert A.shape == (f.m, f.n) and np.array_equal(A.colptr, p) and np.array_equal(A.rowval, i)
        assert np.array_equal(A.nzval.view(np.int64), v.view(np.int64))
        D.set_slots(2)
        D.set_values(2.0 * v, slot=1)
        assert np.array_equal(D.to_csc(1).nzval.view(np.int64), (2.0 * v).view(np.int64))
        assert np.array_equal(D.to_csc(0).nzval.view(np.int64), v.view(np.int64))
        D.select(1)
        assert np.array_equal(D.to_csc().nzval.view(np.int64), (2.0 * v).view(np.int64))
        if f.m == f.n:
            nxt = LR.random_lines(f.n, 12)
            D.set_lines(nxt)
            assert np.array_equal(D.lines, nxt)
            D.set_lines(None)
            assert D.lines is None


# ---- the assembler ---------------------------------------------------------------------------------------------------------------------------------
def test_assembler_submatrix_is_the_operators_and_leaves_the_bookkeeping_alone():
    import torch

    import otmb_amd
    from otmb_amd import synthetic
    from otmb_amd.device import DeviceAssembler

    g = synthetic.make_grid(12, 10, 6, seed=4, rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev, lon_vertices=g.lon_vertices,
                                  lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    op = asm.operator("T")
    N = asm.N
    mask = torch.ones(N, dtype=torch.bool, device=asm.device)
    mask[::3] = False
    idx = torch.nonzero(mask).flatten()
    ops, replans = dict(asm._ops), asm.op_replans
    A = asm.submatrix(mask)
    assert asm._ops == ops and asm._ops["T"].op is op and asm.op_replans == replans
    B = op.submatrix(idx)
    Cc = asm.submatrix(mask, idx[: len(idx) // 2])
    Dd = op.submatrix(idx, idx[: len(idx) // 2])
    torch.cuda.synchronize()
    try:
        for one, two in ((A, B), (Cc, Dd)):
            assert one.shape == two.shape and one.nnz == two.nnz
            for a, b in zip(one.to_csc(), two.to_csc()):
                assert torch.equal(a.view(torch.int64), b.view(torch.int64))
            X = torch.from_numpy(np.random.default_rng(59).standard_normal((3, one.shape[1]))).to(asm.device).t()  # (column-major n x 3)
            assert torch.equal(one.mul(X).view(torch.int64), two.mul(X).view(torch.int64))
        assert A.lines is not None and torch.equal(A.lines, B.lines) and Cc.lines is None
        # the lines are the grid's water columns, restricted; the matrix is the restatement's
        want = SUB.restrict_lines(asm.vertical_lines().cpu().numpy(), idx.cpu().numpy())
        assert np.array_equal(A.lines.cpu().numpy(), want)
        cp, rv, nz = (t.cpu().numpy() for t in op.to_csc())
        cpc, rvc, src = SUB.submatrix_ref(N, N, cp, rv, idx.cpu().numpy(), idx.cpu().numpy())
        a = [t.cpu().numpy() for t in A.to_csc()]
        assert np.array_equal(a[0], cpc) and np.array_equal(a[1], rvc) and np.array_equal(a[2].view(np.int64), nz[src].view(np.int64))
        # a refresh from the assembler's operator after its values changed
        op.set_values_dev(torch.from_numpy(2.0 * nz).to(asm.device))
        A.take_values(op)
        assert np.array_equal(A.to_csc()[2].cpu().numpy().view(np.int64), (2.0 * nz[src]).view(np.int64))
    finally:
        for D in (A, B, Cc, Dd):
            D.close()


# ---- the Dirichlet recipe ----------------------------------------------------------------------------------------------------------------------------
def test_dirichlet_blocks_solve_the_interior_system(oracle):
    """x_B prescribed on the level-1 cells of odd_nx_fold: A_II·x_I = 1 - A_IB·x_B through dirichlet_blocks, against the residual bound of the
    solver's tests and, for x_B = 0, against the dense answer of tests/test_submatrix_ref.py within that bound."""
    import scipy.sparse as sp

    api = _api()
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    p, i, v = T
    A = sp.csc_matrix((v, np.asarray(i) - 1, np.asarray(p) - 1), shape=(N, N))
    rtol = 1e-10
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))) as P:
        P.set_lines(nxt)
        bmask = np.zeros(N, dtype=bool)
        bmask[:nsurf] = True
        AII, AIB, inner, bnd = api.dirichlet_blocks(P, bmask)
        try:
            assert np.array_equal(inner, np.arange(nsurf, N)) and np.array_equal(bnd, np.arange(nsurf))
            assert AII.shape == (N - nsurf, N - nsurf) and AIB.shape == (N - nsurf, nsurf) and AII.lines is not None and AIB.lines is None
            Aii = A[inner][:, inner]
            for what, xB in (("x_B = 0", np.zeros(nsurf)), ("x_B random", np.random.default_rng(53).uniform(0.0, 2.0, nsurf))):
                rhs = np.ones(len(inner)) - AIB.mul(xB)
                xI, info = AII.solve(rhs, precond="lines", rtol=rtol, maxiter=5000)
                print(what, info)
                assert info.converged.all(), info
                (res, bound), = R.residual_check(Aii, xI, rhs, None, 0.0, False, rtol)
                print(what, "residual", res, "bound", bound)
                assert res <= bound
                x = np.concatenate([xB, xI])  # rows I of the whole system: (A·x)_I = 1
                assert np.linalg.norm((A @ x)[inner] - 1.0) <= bound + 2 * (R.longest(A, False) + 3) * R.EPS * np.linalg.norm(abs(A) @ np.abs(x))
                if what == "x_B = 0":
                    xd = np.linalg.solve(Aii.toarray(), np.ones(len(inner)))
                    (resd, boundd), = R.residual_check(Aii, xd, rhs, None, 0.0, False, rtol)
                    gap = np.linalg.norm(Aii @ (xI - xd))
                    print("dense answer: residual", resd, "bound", boundd, "‖A_II·(x - x_dense)‖", gap)
                    assert resd <= boundd and gap <= bound + boundd
        finally:
            AII.close()
            AIB.close()
