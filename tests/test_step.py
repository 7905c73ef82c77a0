"""Value slots and θ-steps on the device (csrc/otmb_step.hip, the slots of csrc/otmb_spmv.hip; otmb_op_set_slots, otmb_op_select_slot,
otmb_op_set_values_slot, otmb_op_step): step() has the BITS of the composition of public calls the header states -- select / mul / the
elementwise line in numpy (tests/step_ref.py: rhs) / solve(x0 = the state) on the same operator -- with slots that are revisited, so the
preconditioner kept per slot is used; the slots' own rules; every refusal leaves X and the operator as they were."""
import ctypes as C

import numpy as np
import pytest

import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from spmv_ref import bits

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAXITER = 5000
NSTEPS, FIRST = 7, 2


def _csc(n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(n, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _same_bits(a, b, what):
    assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), what


def _start(N, k, seed):
    X = np.ones((N, k), order="F")
    X[:, 1:] = np.random.default_rng(seed).standard_normal((N, k - 1))
    return X


def _operator(n, p, i, v, nxt=None, seed=1):
    """A DeviceOperator with the three slots of the tests (T, 0.5·T, T perturbed by ±10 %) and, optionally, lines."""
    import otmb_amd.api as api

    D = api.DeviceOperator(_csc(n, p, i, v))
    D.set_slots(3)
    for s, vals in enumerate(SR.slot_values(v, seed=seed)):
        D.set_values(vals, slot=s)
    if nxt is not None:
        D.set_lines(nxt)
    return D


def _compose(D, X, *, dt, theta, nsteps, first_slot, source, d, adjoint, precond, rtol=RTOL, maxiter=MAXITER):
    """The header's contract in public calls.  -> (X, steps_done, per step (iterations, relres, reason))."""
    nslots, selected = D.slots
    sigma, _ = SR.constants(dt, theta)
    X = np.array(X, dtype=np.float64, order="F")
    done, rows = 0, []
    for t in range(nsteps):
        D.select((first_slot + t) % nslots)
        W = None if theta == 1 else D.mul(X, adjoint=adjoint)
        B = SR.rhs(X, W, source, d, dt, theta)
        X, info = D.solve(B, d=d, sigma=sigma, rtol=rtol, maxiter=maxiter, x0=X, adjoint=adjoint, precond=precond)
        rows.append((info.iterations, info.relres, info.reason))
        if not info.converged.all():
            break
        done = t + 1
    D.select(selected)
    return X, done, rows


def _check_against_composition(D, X0, what, **kw):
    Xs, info = D.step(X0, rtol=RTOL, maxiter=MAXITER, **kw)
    Xc, done, rows = _compose(D, X0, **kw)
    print(what, "steps_done", info.steps_done, "iterations", info.iterations.tolist())
    assert info.status == 0 and info.steps_done == done == kw["nsteps"], (what, info)
    _same_bits(Xs, Xc, what)
    assert len(rows) == len(info.iterations)
    for t, (it, rr, why) in enumerate(rows):
        assert np.array_equal(info.iterations[t], it) and info.reason[t] == why, (what, t)
        _same_bits(info.relres[t], rr, (what, t, "relres"))
    return Xs, info


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117): the whole cross product of the step's arguments runs here."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    D = _operator(N, *T, nxt=nxt)
    yield D, N, R.shift("age", N, nsurf)[0]
    D.close()


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_step_has_the_bits_of_the_public_calls(small, theta, adjoint, precond):
    """k = 1, 3, 7 (register blocks 1; 2 + 1; 4 + 2 + 1) x d none / the age d x source none / random, 7 steps from slot 2 over 3 slots (every
    slot is visited again: the kept preconditioner), δt = one month; and column c of k = 7 has the bits of that column stepped alone."""
    D, N, dage = small
    S7 = np.asfortranarray(np.random.default_rng(11).standard_normal((N, 7)) * 1e-7)
    X7 = _start(N, 7, 12)
    for k in (1, 3, 7):
        for d in (None, dage):
            for S in (None, S7[:, :k]):
                kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, source=S, d=d, adjoint=adjoint, precond=precond)
                Xs, info = _check_against_composition(D, X7[:, :k], (theta, adjoint, precond, k, d is not None, S is not None), **kw)
                if k == 7 and d is not None and S is not None:
                    for c in (0, 3, 6):
                        kw1 = dict(kw, source=S7[:, c])
                        xc, ic = D.step(X7[:, c], rtol=RTOL, maxiter=MAXITER, **kw1)
                        _same_bits(xc, Xs[:, c], ("column alone", c))
                        assert np.array_equal(ic.iterations[:, 0], info.iterations[:, c])
    assert D.slots == (3, 0)  # the selection is the caller's


@pytest.mark.parametrize("name", ["tiny_tripolar", "small_rho3d"])
def test_step_on_larger_grids(oracle, name):
    """N = 429 and 6962 (several workgroups and slices): θ = 0.5 and 1, A and Aᵀ, lines, the age d, a source, k = 7; every step's state
    also meets the float64 residual bound of the solver's tests for its own system."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    p, i, v = T
    d = R.shift("age", N, nsurf)[0]
    S = np.asfortranarray(np.random.default_rng(21).standard_normal((N, 7)) * 1e-7)
    X0 = _start(N, 7, 22)
    with _operator(N, p, i, v, nxt=nxt) as D:
        for theta, adjoint in ((0.5, False), (0.5, True), (1.0, False)):
            kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, source=S, d=d, adjoint=adjoint, precond="lines")
            _check_against_composition(D, X0, (name, theta, adjoint), **kw)
        # one step, checked without the library's word: the system's residual in float64
        Xs, info = D.step(X0, dt=SR.MONTH, theta=0.5, nsteps=1, first_slot=1, source=S, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines")
        values = SR.slot_values(v, seed=1)
        from spmv_ref import spmv_ref

        B = SR.rhs(X0, spmv_ref(N, N, p, i, values[1], X0), S, d, SR.MONTH, 0.5)
        for c, (res, bound) in enumerate(R.residual_check(R.csc_of(N, N, p, i, values[1]), Xs, B, d, SR.constants(SR.MONTH, 0.5)[0], False, RTOL)):
            print(name, "column", c, "residual", res, "bound", bound)
            assert res <= bound


@pytest.mark.parametrize("adjoint", [False, True])
def test_step_with_a_long_row(adjoint):
    """solve_ref.arrow(5000): row 1 (and column 1) has 5000 entries -- the long-row workgroup of the right-hand side's kernel, θ = 0.5."""
    n = 5000
    p, i, v = R.arrow(n)
    S = np.asfortranarray(np.random.default_rng(31).standard_normal((n, 3)))
    with _operator(n, p, i, v) as D:
        kw = dict(dt=SR.MONTH, theta=0.5, nsteps=NSTEPS, first_slot=FIRST, source=S, d=None, adjoint=adjoint, precond="jacobi")
        _check_against_composition(D, _start(n, 3, 32), ("arrow", adjoint), **kw)


def test_slots_grow_shrink_and_one_slot_is_todays_operator():
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    n = 257
    p, i, v = R.dominant(n)
    X = _start(n, 3, 41)
    with api.DeviceOperator(_csc(n, p, i, v)) as D, api.DeviceOperator(_csc(n, p, i, v)) as E:
        assert D.slots == (1, 0)
        # one slot: set_values / mul / solve give the bits of a second operator on which no slot call was ever made
        D.set_slots(1)
        D.select(0)
        D.set_values(2.0 * v)
        E.set_values(2.0 * v)
        for adjoint in (False, True):
            _same_bits(D.mul(X, adjoint=adjoint), E.mul(X, adjoint=adjoint), ("one slot: mul", adjoint))
            xd, idd = D.solve(X, sigma=0.5, adjoint=adjoint)
            xe, ie = E.solve(X, sigma=0.5, adjoint=adjoint)
            _same_bits(xd, xe, ("one slot: solve", adjoint))
            assert np.array_equal(idd.iterations, ie.iterations)
        # growing copies the SELECTED slot into every new one
        D.set_slots(3)
        assert D.slots == (3, 0)
        want = E.mul(X)
        for s in (1, 2):
            D.select(s)
            _same_bits(D.mul(X), want, ("a new slot is a copy", s))
            _same_bits(D.mul(X, adjoint=True), E.mul(X, adjoint=True), ("a new slot is a copy, CSC side", s))
        D.set_values(3.0 * v)  # writes the selected slot (2) only
        E.set_values(3.0 * v)
        _same_bits(D.mul(X), E.mul(X), "set_values writes the selected slot")
        D.select(0)
        _same_bits(D.mul(X), want, "slot 0 kept its values")
        D.set_values(v, slot=1)  # whichever is selected
        assert D.slots == (3, 0)
        E.set_values(v)
        D.select(1)
        _same_bits(D.mul(X), E.mul(X), "set_values(slot=1)")
        D.select(2)
        D.set_slots(5)  # growing keeps the slots and copies slot 2
        assert D.slots == (5, 2)
        D.select(4)
        E.set_values(3.0 * v)
        _same_bits(D.mul(X), E.mul(X), "slot 4 is a copy of slot 2")
        # shrinking below the selected slot selects slot 0
        D.set_slots(2)
        assert D.slots == (2, 0)
        _same_bits(D.mul(X), want, "slot 0 after shrinking")
        D.select(1)
        D.set_slots(2)
        assert D.slots == (2, 1)
        # refusals: the operator stays as it was
        for call in (lambda: D.set_slots(0), lambda: D.set_slots(-3), lambda: D.select(2), lambda: D.select(-1), lambda: D.set_values(v, slot=2),
                     lambda: D.set_values(v, slot=-1), lambda: D.set_values(v[:-1], slot=0), lambda: D.set_values(v[:-1])):
            with pytest.raises(OtmbError) as e:
                call()
            assert e.value.name == "INVALID_ARG", str(e.value)
            assert D.slots == (2, 1)
        E.set_values(v)
        _same_bits(D.mul(X), E.mul(X), "after the refusals")


def _step_c(D, X, ldx, k, *, S=None, lds=None, d=None, dt=SR.MONTH, theta=1.0, nsteps=NSTEPS, first_slot=0, rtol=RTOL, maxiter=MAXITER, precond=0,
            adjoint=0, nrep=None):
    """otmb_op_step through the C ABI.  -> (status, steps_done, iters, relres, reason) with the report arrays preset to sentinels."""
    from otmb_amd import capi

    nrep = max(nsteps, 1) if nrep is None else nrep
    it, rr, why = np.full((nrep, k), -7, np.int64), np.full((nrep, k), 7.25), np.full((nrep, k), -7, np.int32)
    done = C.c_int64(-7)
    rc = capi.lib().otmb_op_step(D.handle, adjoint, k, None if d is None else d.ctypes.data, float(dt), float(theta), nsteps, first_slot,
                                 None if S is None else S.ctypes.data, 0 if lds is None else lds, None if X is None else X.ctypes.data, ldx,
                                 float(rtol), maxiter, precond, C.byref(done), it.ctypes.data, rr.ctypes.data, why.ctypes.data)
    return rc, done.value, it, rr, why


def test_leading_dimensions_and_sentinel_rows(small):
    """ldx, lds > n: the padding rows of S are not read (NaN), those of X are not written."""
    D, N, dage = small
    X0 = _start(N, 3, 51)
    S = np.asfortranarray(np.random.default_rng(52).standard_normal((N, 3)) * 1e-7)
    for theta, pc in ((0.5, 1), (1.0, 0)):
        Xp = np.full((N + 5, 3), 7.25, order="F")
        Xp[:N] = X0
        Sp = np.full((N + 3, 3), np.nan, order="F")
        Sp[:N] = S
        rc, done, it, rr, why = _step_c(D, Xp, N + 5, 3, S=Sp, lds=N + 3, d=dage, theta=theta, first_slot=FIRST, precond=pc)
        assert rc == 0 and done == NSTEPS and (why == 0).all() and (it >= 0).all()
        assert (Xp[N:] == 7.25).all() and np.isnan(Sp[N:]).all()
        want, _ = D.step(X0, dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, source=S, d=dage, rtol=RTOL, maxiter=MAXITER,
                         precond=("jacobi", "lines")[pc])
        _same_bits(Xp[:N], want, ("padded", theta))


def test_refusals_leave_x_and_the_operator_unchanged(small):
    import otmb_amd.api as api
    from otmb_amd import capi

    D, N, dage = small
    X0 = _start(N, 2, 61)
    S = np.asfortranarray(np.ones((N, 2)))
    before = D.mul(X0)
    bad = [dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(theta=0.0), dict(theta=1.5), dict(theta=float("nan")),
           dict(nsteps=-1), dict(first_slot=3), dict(first_slot=-1), dict(rtol=0.0), dict(maxiter=-1), dict(precond=2), dict(precond=-1),
           dict(S=S, lds=N - 1)]
    for kw in bad:
        X = X0.copy(order="F")
        rc, done, it, rr, why = _step_c(D, X, N, 2, **kw)
        assert rc == 11, kw
        assert np.array_equal(X, X0) and (it == -7).all() and D.slots == (3, 0), kw
    # two bad arguments at once: the complaint is the first in the checks' order
    for kw, first in ((dict(rtol=0.0, dt=0.0), "rtol must be > 0"), (dict(theta=0.0, first_slot=99), "theta must be in (0, 1]"),
                      (dict(nsteps=-1, first_slot=99), "nsteps must be >= 0")):
        X = X0.copy(order="F")
        assert _step_c(D, X, N, 2, **kw)[0] == 11, kw
        assert capi.lib().otmb_last_error(D.ctx.handle).decode() == f"{capi.lib().otmb_status_string(11).decode()}: {first}", kw
        assert np.array_equal(X, X0) and D.slots == (3, 0), kw
    X = X0.copy(order="F")
    assert _step_c(D, X, N - 1, 2)[0] == 11 and _step_c(D, X, N, 0)[0] == 11 and _step_c(D, None, N, 2)[0] == 11
    assert capi.lib().otmb_op_step(None, 0, 2, None, 1.0, 1.0, 1, 0, None, 0, X.ctypes.data, N, RTOL, 10, 0, None, None, None, None) == 11
    assert capi.lib().otmb_op_step(D.handle, 0, 2, None, 1.0, 1.0, 1, 0, None, 0, X.ctypes.data, N, RTOL, 10, 0, None, None, None, None) == 11
    assert np.array_equal(X, X0)
    # nsteps = 0: OTMB_OK, nothing but steps_done is written
    rc, done, it, rr, why = _step_c(D, X, N, 2, nsteps=0)
    assert rc == 0 and done == 0 and np.array_equal(X, X0) and (it == -7).all() and (rr == 7.25).all() and (why == -7).all()
    # lines on an operator without lines, a rectangular operator
    p, i, v = R.dominant(257)
    with api.DeviceOperator(_csc(257, p, i, v)) as E:
        Y = _start(257, 2, 62)
        Y0 = Y.copy(order="F")
        assert _step_c(E, Y, 257, 2, precond=1)[0] == 11 and np.array_equal(Y, Y0)
    rect = api.SparseMatrixCSC(3, 2, np.array([1, 2, 3], dtype=np.int64), np.array([1, 2], dtype=np.int64), np.array([1.0, 1.0]))
    with api.DeviceOperator(rect) as Q:
        Y = np.ones((3, 1), order="F")
        assert _step_c(Q, Y, 3, 1)[0] == 11 and (Y == 1.0).all()
    _same_bits(D.mul(X0), before, "the operator after the refusals")


def test_a_step_that_does_not_converge_ends_the_call(small, oracle):
    """maxiter = 1 with Jacobi on the month system: OTMB_ERR_NOT_CONVERGED at step 0, steps_done = 0, that step's reasons, its last iterates in
    X; the later steps' report entries are not written.  And a failure at a later step: slot 0 holds 1e-6·T, whose month system is the
    identity but for 1e-3 (a handful of Jacobi iterations), slot 1 holds T, which needs about 190 (tests/test_solve_lines_ref.py's table):
    with maxiter = 20 the call completes step 0 and ends at step 1."""
    import otmb_amd.api as api

    D, N, dage = small
    X0 = _start(N, 2, 71)
    X = X0.copy(order="F")
    rc, done, it, rr, why = _step_c(D, X, N, 2, maxiter=1, first_slot=FIRST)
    assert rc == 19 and done == 0
    assert (why[0] == 1).all() and (it[0] == 1).all() and (rr[0] > RTOL).all()
    assert (it[1:] == -7).all() and (why[1:] == -7).all() and (rr[1:] == 7.25).all()
    Xc, cdone, rows = _compose(D, X0, dt=SR.MONTH, theta=1.0, nsteps=NSTEPS, first_slot=FIRST, source=None, d=None, adjoint=False,
                               precond="jacobi", maxiter=1)
    assert cdone == 0 and rows[0][2] == ("maxiter", "maxiter")
    _same_bits(X, Xc, "the failing step's last iterates")
    _same_bits(rr[0], rows[0][1], "relres")
    # the Python layer reports it as solve does: no exception
    Xs, info = D.step(X0, dt=SR.MONTH, nsteps=NSTEPS, first_slot=FIRST, maxiter=1)
    assert info.status == 19 and info.steps_done == 0 and info.reason == (("maxiter", "maxiter"),) and not info.converged.any()
    _same_bits(Xs, Xc, "through the Python layer")
    T, _, _, _ = LR.grid(oracle, "odd_nx_fold")
    with api.DeviceOperator(_csc(N, T[0], T[1], 1e-6 * T[2])) as E:
        E.set_slots(2)
        E.set_values(T[2], slot=1)
        kw = dict(dt=SR.MONTH, theta=1.0, nsteps=4, first_slot=0, source=None, d=None, adjoint=False, precond="jacobi")
        Xs, info = E.step(X0, rtol=RTOL, maxiter=20, **kw)
        Xc, cdone, rows = _compose(E, X0, maxiter=20, **kw)
        print("a later step fails:", info)
        assert info.status == 19 and info.steps_done == cdone == 1 and len(info.iterations) == 2
        assert info.converged[0].all() and "maxiter" in info.reason[1]
        _same_bits(Xs, Xc, "a later step fails: its last iterates")
        assert np.array_equal(info.iterations[1], rows[1][0])


def test_the_host_route_keeps_the_failing_steps_message(small, oracle):
    """The later failure of the test above (slot 0 holds 1e-6·T, slot 1 holds T, maxiter = 20: step 1 does not converge) through
    otmb_op_step: after X has come back and the stream was waited for, the context's message is still the solver's report, with the step's
    suffix, and X has the bits the device route leaves on the device."""
    import torch

    import otmb_amd.api as api
    from otmb_amd import capi, device

    _, N, _ = small
    X0 = _start(N, 2, 71)
    T, _, _, _ = LR.grid(oracle, "odd_nx_fold")
    kw = dict(dt=SR.MONTH, theta=1.0, nsteps=4, first_slot=0, rtol=RTOL, maxiter=20, precond="jacobi")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(torch.device("cuda", 0))
    ctx = device.DeviceAssembler(0).ctx
    with api.DeviceOperator(_csc(N, T[0], T[1], 1e-6 * T[2])) as E, \
            device.Operator(ctx, N, N, t(T[0], np.int64), t(T[1], np.int64), t(1e-6 * T[2], np.float64)) as O:
        E.set_slots(2)
        E.set_values(T[2], slot=1)
        O.set_slots(2)
        O.set_values_dev(t(T[2], np.float64), slot=1)
        Xh, ih = E.step(X0, **kw)
        msg = capi.lib().otmb_last_error(E.ctx.handle).decode()
        print("host route:", ih.status, ih.steps_done, msg)
        assert ih.status == capi.NOT_CONVERGED and ih.steps_done == 1
        assert msg.startswith("solve: not converged") and msg.endswith("(step 1, slot 1)"), msg
        Xg, ig = O.step(t(X0.T, np.float64).t(), **kw)
        assert ig.status == capi.NOT_CONVERGED and ig.steps_done == 1
        _same_bits(Xh, Xg.cpu().numpy(), "the host route's X against the device route's")


def test_a_singular_slot_stops_the_call_before_its_step():
    """[[1, 4], [1, 1]] + σ·I with σ = 1 (δt = 1, θ = 1) on the line 1 -> 2: m_2 = 1 / 2, piv_2 = 2 - (1 / 2)·4 = 0 exactly (the matrix of
    tests/test_solve_lines.py, shifted).  It sits in slot 1: the call ends at step 1 with OTMB_ERR_SINGULAR_PRECONDITIONER, steps_done = 1,
    and X is the state after step 0."""
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    p, i = np.array([1, 3, 5, 6]), np.array([1, 2, 1, 2, 3])
    regular, singular = np.array([3.0, 1.0, 1.0, 3.0, 1.0]), np.array([1.0, 1.0, 4.0, 1.0, 1.0])
    with api.DeviceOperator(_csc(3, p, i, regular)) as Z:
        Z.set_lines(np.array([2, 0, 0]))
        Z.set_slots(2)
        Z.set_values(singular, slot=1)
        X0 = np.asfortranarray(np.array([[1.0], [2.0], [3.0]]))
        X = X0.copy(order="F")
        rc, done, it, rr, why = _step_c(Z, X, 3, 1, dt=1.0, theta=1.0, nsteps=3, precond=1)
        assert rc == 18 and done == 1 and why[0, 0] == 0 and (it[1:] == -7).all()
        want, info = Z.solve(SR.rhs(X0, None, None, None, 1.0, 1.0), sigma=1.0, x0=X0, precond="lines", rtol=RTOL, maxiter=MAXITER)
        assert info.converged.all()
        _same_bits(X, want, "the state after step 0")
        with pytest.raises(OtmbError) as e:
            Z.step(X0, dt=1.0, nsteps=3, precond="lines")
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "pivot[2]" in str(e.value) and "step 1" in str(e.value), str(e.value)
        # at step 0 nothing of X is touched
        X = X0.copy(order="F")
        rc, done, it, rr, why = _step_c(Z, X, 3, 1, dt=1.0, theta=1.0, nsteps=3, first_slot=1, precond=1)
        assert rc == 18 and done == 0 and np.array_equal(X, X0) and (it == -7).all()
        assert Z.slots == (2, 0)


def test_the_device_route_has_the_same_bits():
    """device.Operator.step on torch tensors (otmb_op_step_dev) against api.DeviceOperator.step (otmb_op_step), and slots through it."""
    import torch

    import otmb_amd.api as api
    from otmb_amd import device

    n = 257
    p, i, v = R.dominant(n)
    dev = torch.device("cuda", 0)
    ctx = device.DeviceAssembler(0).ctx  # (on torch's stream)
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    X0 = _start(n, 3, 81)
    S = np.asfortranarray(np.random.default_rng(82).standard_normal((n, 3)))
    d = np.random.default_rng(83).uniform(0.0, 1.0, n)
    with _operator(n, p, i, v, nxt=LR.random_lines(n, 3)) as D, device.Operator(ctx, n, n, t(p, np.int64), t(i, np.int64), t(v, np.float64)) as O:
        O.set_slots(3)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            O.set_values_dev(t(vals, np.float64), slot=s)
        O.set_lines(t(LR.random_lines(n, 3), np.int64))
        assert O.slots == (3, 0)
        Xd = t(X0.T, np.float64).t()  # column-major on the device
        Sd = t(S.T, np.float64).t()
        for theta, adjoint, precond in ((0.5, False, "lines"), (0.5, True, "jacobi"), (1.0, False, "lines")):
            kw = dict(dt=2.0, theta=theta, nsteps=NSTEPS, first_slot=FIRST, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
            Xh, ih = D.step(X0, source=S, d=d, **kw)
            Xg, ig = O.step(Xd, source=Sd, d=t(d, np.float64), **kw)
            assert ih.steps_done == ig.steps_done == NSTEPS
            _same_bits(Xg.cpu().numpy(), Xh, ("device route", theta, adjoint, precond))
            assert np.array_equal(ig.iterations, ih.iterations)
            _same_bits(Xd.cpu().numpy(), X0, "X is not modified")
        O.select(1)
        D.select(1)
        _same_bits(O.mul(Xd).cpu().numpy(), D.mul(X0), "select on the device route")


# ---- the step without the library's word -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_grids(oracle):
    """Per grid: the operator with the tests' three slots and the grid's water columns, and what scipy needs to judge it."""
    made = {}

    def get(name):
        if name not in made:
            T, N, nsurf, nxt = LR.grid(oracle, name)
            made[name] = (_operator(N, *T, nxt=nxt), N, T, R.shift("age", N, nsurf)[0])
        return made[name]

    yield get
    for D, *_ in made.values():
        D.close()


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", ["odd_nx_fold", "tiny_tripolar"])
def test_every_step_against_scipy_and_the_chain_against_one_call(chain_grids, name, theta, adjoint, precond):
    """Four steps of one month from slot 2 over three slots, the age d, a source of scale 1e-7, k = 3, as four nsteps = 1 calls fed into
    each other with first_slot advanced by hand: every pair (X_{t-1}, X_t) meets step_ref.step_residual_check -- the θ-method written down
    from the differential equation, in float64 with scipy's matrix of THAT slot, and a bound that is derived there -- which pins the slot
    order, the adjoint, θ = 1, Jacobi and the constants σ, s/θ and (1 - θ)/θ without step_ref.rhs or any call of the library.  Then ONE
    nsteps = 4 call returns X_4's bits and the same iteration rows: the multi-step call is tied to the checked chain."""
    D, N, (p, i, v), d = chain_grids(name)
    values = SR.slot_values(v, seed=1)
    S = np.asfortranarray(np.random.default_rng(91).standard_normal((N, 3)) * 1e-7)
    X0 = _start(N, 3, 92)
    kw = dict(dt=SR.MONTH, theta=theta, source=S, d=d, adjoint=adjoint, precond=precond, rtol=RTOL, maxiter=MAXITER)
    X, rows = X0, []
    for t in range(4):
        slot = (FIRST + t) % 3
        Xn, info = D.step(X, nsteps=1, first_slot=slot, **kw)
        assert info.status == 0 and info.steps_done == 1, (name, t, info)
        rows.append(info.iterations[0])
        A = R.csc_of(N, N, p, i, values[slot])
        for c, (res, bound) in enumerate(SR.step_residual_check(A, X, Xn, S, d, SR.MONTH, theta, adjoint, RTOL)):
            print(name, theta, adjoint, precond, "step", t, "slot", slot, "column", c, "iterations", int(info.iterations[0][c]), "residual", res,
                  "bound", bound)
            assert res <= bound, (name, t, c, res, bound)
        X = Xn
    X4, info = D.step(X0, nsteps=4, first_slot=FIRST, **kw)
    assert info.status == 0 and info.steps_done == 4, info
    _same_bits(X4, X, (name, "one call of four steps"))
    assert np.array_equal(np.asarray(info.iterations), np.asarray(rows)), (info.iterations, rows)
    assert D.slots == (3, 0)


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
def test_a_steady_state_is_a_fixed_point_of_the_step(oracle, precond):
    """(diag(d) + A)·x* = s (the steady ideal age on odd_nx_fold: s = 1, x* by scipy's LU with one refinement): in exact arithmetic
    b - M·x* = (s - (diag(d) + A)·x*)/θ whatever σ is, so three steps from x* over three slots that all hold T take NO iteration and return
    x*'s bits, for θ = 1, 0.5, 0.25 and δt = a day, a month.  A wrong s/θ, (1 - θ)/θ or σ on either side of the system breaks it, and nothing
    here goes through step_ref.rhs.  tests/test_step_ref.py (the test of the same name) shows on the CPU that every pair starts a factor 100
    below rtol and that no summation order can close that margin: all six pairs pass there, none is dropped."""
    import otmb_amd.api as api
    from test_step_ref import FIXED_POINT_PAIRS, steady_age

    T, N, nxt, d, s, x = steady_age(oracle)
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_slots(3)  # (every new slot is a copy of the selected one: three times T)
        D.set_lines(nxt)
        for theta, dt in FIXED_POINT_PAIRS:
            X, info = D.step(x, dt=dt, theta=theta, nsteps=3, first_slot=0, source=s, d=d, rtol=RTOL, maxiter=MAXITER, precond=precond)
            print("theta", theta, "dt", dt, precond, "iterations", np.asarray(info.iterations).tolist(), "relres", np.asarray(info.relres).tolist())
            assert info.status == 0 and info.steps_done == 3, (theta, dt, info)
            assert (np.asarray(info.iterations) == 0).all(), (theta, dt, info.iterations)
            _same_bits(X, x, (theta, dt, "x* is a fixed point"))


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("adjoint", [0, 1])
def test_a_nan_column_stops_the_call_and_spares_its_neighbours(small, adjoint, precond):
    """k = 3 with one NaN in column 1 of the start, θ = 0.5, nsteps = 3: OTMB_ERR_NOT_CONVERGED at step 0, steps_done = 0, reasons
    (converged, nonfinite, converged); column 1 is left as it was, columns 0 and 2 have the bits and the iterations of a clean one-step call
    on those two columns, and the report rows of the steps that never ran keep their sentinels."""
    D, N, dage = small
    X0 = _start(N, 3, 95)
    X0[5, 1] = np.nan
    S = np.asfortranarray(np.random.default_rng(96).standard_normal((N, 3)) * 1e-7)
    X = X0.copy(order="F")
    rc, done, it, rr, why = _step_c(D, X, N, 3, S=S, lds=N, d=dage, theta=0.5, nsteps=3, first_slot=FIRST, precond=precond, adjoint=adjoint)
    assert rc == 19 and done == 0, (rc, done)
    assert why[0].tolist() == [0, 3, 0], why
    assert it[0, 1] == 0 and np.isnan(rr[0, 1]) and (rr[0, [0, 2]] <= RTOL).all(), (it, rr)
    assert (it[1:] == -7).all() and (why[1:] == -7).all() and (rr[1:] == 7.25).all()
    _same_bits(X[:, 1], X0[:, 1], "the NaN column is left as it was")
    clean, info = D.step(X0[:, [0, 2]], dt=SR.MONTH, theta=0.5, nsteps=1, first_slot=FIRST, source=S[:, [0, 2]], d=dage, rtol=RTOL, maxiter=MAXITER,
                         precond=("jacobi", "lines")[precond], adjoint=bool(adjoint))
    assert info.status == 0 and info.steps_done == 1
    _same_bits(X[:, [0, 2]], clean, "the clean columns")
    assert np.array_equal(it[0, [0, 2]], info.iterations[0])
    assert D.slots == (3, 0)
