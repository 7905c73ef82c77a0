"""GPU: otmb_op_step_obs[_dev] (csrc/otmb_step.hip's one loop, csrc/otmb_observe.hip's pass): step(..., observe=W, time_weights=w) returns the
X and every StepInfo field of plain step bit for bit, observations[t] with the bits of tests/observe_ref.py on the state that t + 1 single
steps of the existing step give, and mean with the bits of the host fold over those states.

tiny_tripolar's T (N = 429) with the tests' three slots, nsteps = 5 so the slots wrap, k = 3, q = 2, θ = 1 and 0.5, A and Aᵀ, Jacobi and lines;
observations only, mean only and neither (step's own path); a call that stops early; the C entry on sentinel-filled arrays; the device
route; DeviceAssembler.step_tracers; and one test of use: the inventory of a tracer under a mass-conserving T."""
import ctypes as C
import math

import numpy as np
import pytest

import observe_ref as OR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _csc, _operator, _same_bits, _start

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
NSTEPS, FIRST, K, Q = 5, 2, 3, 2
TW = np.array([0.125, 0.25, 0.0, 0.5, 0.125])  # (a zero weight: the product still enters the fold)


@pytest.fixture(scope="module")
def tiny(oracle):
    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    D = _operator(N, *T, nxt=nxt)
    rng = np.random.default_rng(41)
    W = np.asfortranarray(rng.uniform(0.5, 1.5, (N, Q)))
    S = np.asfortranarray(rng.standard_normal((N, K)) * 1e-7)
    yield D, N, T, nxt, R.shift("age", N, nsurf)[0], W, S, _start(N, K, 42)
    D.close()


def _chain(D, X0, nsteps, first_slot, **kw):
    """The states after 1, 2, ... single steps of the existing step."""
    states, X = [], X0
    for t in range(nsteps):
        X, info = D.step(X, nsteps=1, first_slot=(first_slot + t) % D.slots[0], **kw)
        assert info.status == 0 and info.steps_done == 1, (t, info)
        states.append(X)
    return states


def _same_info(a, b, what):
    assert (a.status, a.steps_done, a.reason) == (b.status, b.steps_done, b.reason), what
    assert np.array_equal(a.iterations, b.iterations) and np.array_equal(a.converged, b.converged), what
    _same_bits(a.relres, b.relres, (what, "relres"))


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_record_has_the_bits_of_single_steps_and_the_state_those_of_step(tiny, theta, adjoint, precond):
    D, N, T, nxt, d, W, S, X0 = tiny
    kw = dict(dt=SR.MONTH, theta=theta, source=S, d=d, adjoint=adjoint, precond=precond, rtol=RTOL, maxiter=MAXITER)
    what = (theta, adjoint, precond)
    Xp, ip = D.step(X0, nsteps=NSTEPS, first_slot=FIRST, **kw)  # "neither": step's own path
    assert ip.status == 0 and ip.steps_done == NSTEPS and ip.observations is None and ip.mean is None
    states = _chain(D, X0, NSTEPS, FIRST, **kw)
    _same_bits(states[-1], Xp, (what, "the chain"))
    want_obs = np.stack([OR.observe_ref(W, X).T for X in states])  # (nsteps, k, q)
    want_mean = OR.mean_ref(states, TW)
    for observe, weights in ((W, TW), (W, None), (None, TW)):
        Xo, io = D.step(X0, nsteps=NSTEPS, first_slot=FIRST, observe=observe, time_weights=weights, **kw)
        tag = (what, observe is not None, weights is not None)
        _same_bits(Xo, Xp, (tag, "X"))
        _same_info(io, ip, tag)
        if observe is None:
            assert io.observations is None
        else:
            assert io.observations.shape == (NSTEPS, K, Q)
            _same_bits(io.observations, want_obs, (tag, "observations"))
        if weights is None:
            assert io.mean is None
        else:
            assert io.mean.shape == (N, K)
            _same_bits(io.mean, want_mean, (tag, "mean"))
    assert D.slots == (3, 0)
    # one observer given as n values, a 1-D state: (steps, 1, 1) and n values
    x1, i1 = D.step(X0[:, 1], nsteps=2, first_slot=FIRST, observe=W[:, 1], time_weights=TW[:2], **dict(kw, source=S[:, 1]))
    assert i1.observations.shape == (2, 1, 1) and i1.mean.shape == (N,)
    _same_bits(i1.observations[:, 0, 0], want_obs[:2, 1, 1], (what, "column and observer alone"))
    _same_bits(i1.mean, OR.mean_ref([s[:, 1] for s in states[:2]], TW), (what, "mean of a column alone"))


def test_a_call_that_stops_early_reports_as_step_does(tiny):
    """maxiter = 1: the report is step's, observations keeps steps_done rows and there is no mean of no step."""
    D, N, T, nxt, d, W, S, X0 = tiny
    kw = dict(dt=SR.MONTH, theta=0.5, nsteps=NSTEPS, first_slot=FIRST, source=S, d=d, precond="jacobi", rtol=RTOL, maxiter=1)
    Xp, ip = D.step(X0, **kw)
    Xo, io = D.step(X0, observe=W, time_weights=TW, **kw)
    assert ip.status == 19 and ip.steps_done < NSTEPS
    _same_bits(Xo, Xp, "X")
    _same_info(io, ip, "maxiter = 1")
    assert io.observations.shape == (ip.steps_done, K, Q)
    assert (io.mean is None) == (ip.steps_done == 0)


def _step_obs_c(D, X, k, nsteps, first_slot, q, W, ldw, obs, tw, Xbar, ldm, *, dt=SR.MONTH, theta=1.0, maxiter=MAXITER, precond=0):
    from otmb_amd import capi

    n = D.shape[0]
    it, rr, why = np.full((max(nsteps, 1), k), -7, np.int64), np.full((max(nsteps, 1), k), 7.25), np.full((max(nsteps, 1), k), -7, np.int32)
    done = C.c_int64(-7)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = capi.lib().otmb_op_step_obs(D.handle, 0, k, None, float(dt), float(theta), nsteps, first_slot, None, n, X.ctypes.data, n, RTOL, maxiter, precond,
                                     C.byref(done), it.ctypes.data, rr.ctypes.data, why.ctypes.data, q, ptr(W), ldw, ptr(obs), ptr(tw), ptr(Xbar), ldm)
    return rc, done.value


def test_rows_beyond_steps_done_are_untouched_through_the_c_entry(oracle):
    """Slot 1 is made singular for Jacobi (its diagonal is -σ exactly), so the call from slot 0 ends at step 1 with steps_done = 1: X is
    the state after one step, block 0 of obs is its observation, the other blocks keep their sentinel and Xbar = +0.0 + tw[0]·X_1 under
    untouched padding rows.  With maxiter = 0 no step completes: obs and Xbar are as passed in."""
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    p, i, v = T
    sigma = SR.constants(SR.MONTH, 1.0)[0]
    col = np.repeat(np.arange(1, N + 1), np.diff(p))
    bad = np.array(v, dtype=np.float64)
    bad[i == col] = -sigma
    assert np.bincount(col[i == col], minlength=N + 1)[1:].tolist() == [1] * N  # one stored diagonal entry per column
    rng = np.random.default_rng(43)
    W = np.asfortranarray(rng.uniform(0.5, 1.5, (N, Q)))
    X0 = _start(N, K, 44)
    with api.DeviceOperator(_csc(N, p, i, v)) as D:
        D.set_slots(2)
        D.set_values(bad, slot=1)
        X1, info = D.step(X0, dt=SR.MONTH, nsteps=1, first_slot=0, rtol=RTOL, maxiter=MAXITER)
        assert info.steps_done == 1
        X = X0.copy(order="F")
        obs, Xbar = np.full((3, K, Q), 7.25), np.full((N + 3, K), 7.25, order="F")
        rc, done = _step_obs_c(D, X, K, 3, 0, Q, W, N, obs, TW, Xbar, N + 3)
        assert (rc, done) == (18, 1)
        _same_bits(X, X1, "X after the completed step")
        _same_bits(obs[0], OR.observe_ref(W, X1).T, "block 0")
        assert (obs[1:] == 7.25).all() and (Xbar[N:] == 7.25).all()
        _same_bits(Xbar[:N], OR.mean_ref([X1], TW), "Xbar over the completed step")
        X = X0.copy(order="F")
        obs, Xbar = np.full((3, K, Q), 7.25), np.full((N, K), 7.25, order="F")
        rc, done = _step_obs_c(D, X, K, 3, 0, Q, W, N, obs, TW, Xbar, N, maxiter=0)
        assert (rc, done) == (19, 0) and (obs == 7.25).all() and (Xbar == 7.25).all()
        # q = 0 and no weights: otmb_op_step, bit for bit
        X = X0.copy(order="F")
        rc, done = _step_obs_c(D, X, K, 1, 0, 0, None, 0, None, None, None, 0)
        assert (rc, done) == (0, 1)
        _same_bits(X, X1, "q = 0, no mean")


def test_refusals_write_nothing_and_name_the_call(tiny):
    from otmb_amd import capi

    D, N, T, nxt, d, W, S, X0 = tiny
    nan_w, inf_w = TW[:3].copy(), TW[:3].copy()
    nan_w[1], inf_w[2] = np.nan, np.inf
    Xbar0 = np.full((N, K), 7.25, order="F")
    cases = {"q < 0": (-1, W, N, True, None, False, N), "W null": (Q, None, N, True, None, False, N), "obs null": (Q, W, N, False, None, False, N),
             "ldw < n": (Q, W, N - 1, True, None, False, N), "tw alone": (Q, W, N, True, TW[:3], False, N), "Xbar alone": (Q, W, N, True, None, True, N),
             "NaN weight": (0, None, N, False, nan_w, True, N), "Inf weight": (Q, W, N, True, inf_w, True, N), "ldm < n": (0, None, N, False, TW[:3], True, N - 1)}
    for what, (q, Wc, ldw, has_obs, tw, has_bar, ldm) in cases.items():
        X = X0.copy(order="F")
        obs, Xbar = np.full((3, K, Q), 7.25), Xbar0.copy(order="F")
        rc, done = _step_obs_c(D, X, K, 3, FIRST, q, Wc, ldw, obs if has_obs else None, tw, Xbar if has_bar else None, ldm)
        assert rc == 11 and done == -7, (what, rc, done)
        with pytest.raises(capi.OtmbError, match="otmb_op_step_obs"):
            D.ctx.check(rc)
        _same_bits(X, X0, what)
        assert (obs == 7.25).all() and (Xbar == 7.25).all(), what
    with pytest.raises(capi.OtmbError, match="DimensionMismatch"):
        D.step(X0, dt=SR.MONTH, nsteps=3, time_weights=TW)
    with pytest.raises(capi.OtmbError, match="DimensionMismatch"):
        D.step(X0, dt=SR.MONTH, nsteps=3, observe=W[:-1])
    assert D.slots == (3, 0)
    Xa, ia = D.step(X0, dt=SR.MONTH, nsteps=2, first_slot=FIRST, observe=W, rtol=RTOL, maxiter=MAXITER)  # still usable
    Xb, ib = D.step(X0, dt=SR.MONTH, nsteps=2, first_slot=FIRST, rtol=RTOL, maxiter=MAXITER)
    _same_bits(Xa, Xb, "after the refusals")
    _same_bits(ia.observations[1], OR.observe_ref(W, Xb).T, "the last observation is of the returned state")


def test_the_device_route_has_the_same_bits(tiny):
    """device.Operator.step(observe=, time_weights=) on torch tensors (otmb_op_step_obs_dev), W and X as padded views."""
    import torch

    from otmb_amd import device

    D, N, T, nxt, d, W, S, X0 = tiny
    p, i, v = T
    dev = torch.device("cuda", 0)
    ctx = device.DeviceAssembler(0).ctx
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)

    def padded(a, pad):
        flat = torch.full(((a.shape[0] + pad) * a.shape[1],), float("nan"), dtype=torch.float64, device=dev)
        view = flat.as_strided(a.shape, (1, a.shape[0] + pad))
        view.copy_(t(a))
        return view

    with device.Operator(ctx, N, N, t(p, np.int64), t(i, np.int64), t(v, np.float64)) as O:
        O.set_slots(3)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            O.set_values_dev(t(vals, np.float64), slot=s)
        O.set_lines(t(nxt, np.int64))
        for theta, adjoint, precond, pad in ((0.5, False, "lines", 1), (1.0, True, "jacobi", 2)):
            kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
            Xh, ih = D.step(X0, source=S, d=d, observe=W, time_weights=TW, **kw)
            Xg, ig = O.step(padded(X0, pad), source=padded(S, pad), d=t(d, np.float64), observe=padded(W, pad), time_weights=TW, **kw)
            assert ih.steps_done == ig.steps_done == NSTEPS and np.array_equal(ig.iterations, ih.iterations)
            assert torch.is_tensor(ig.observations) and torch.is_tensor(ig.mean)
            _same_bits(Xg.cpu().numpy(), Xh, ("X", theta))
            _same_bits(ig.observations.cpu().numpy(), ih.observations, ("observations", theta))
            _same_bits(ig.mean.cpu().numpy(), ih.mean, ("mean", theta))
            Xq, iq = O.step(padded(X0, pad), source=padded(S, pad), d=t(d, np.float64), **kw)
            assert iq.observations is None and iq.mean is None
            _same_bits(Xq.cpu().numpy(), Xh, ("plain", theta))
        _same_bits(O.observe(padded(W, 1), padded(X0, 1)).cpu().numpy(), D.observe(W, X0), "observe")


def test_step_tracers_forwards_the_keywords():
    """DeviceAssembler.step_tracers(..., observe=, time_weights=) on kept months agrees with api.DeviceOperator over the same value sets."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _fields, _host, _pair

    g, gm, asm, other, umo, vmo, fill = _pair("small_rho3d")
    del other
    N = asm.N
    fields = _fields(umo, vmo, 2, seed=5)
    months = []
    for m in range(2):
        asm.step(*fields[m], fill)
        asm.keep_slot(m, nslots=2)
        months.append(_host(asm)["T"])
    rng = np.random.default_rng(45)
    X0, W, tw = _start(N, K, 46), np.asfortranarray(rng.uniform(0.5, 1.5, (N, Q))), np.array([0.5, 0.25, 0.25])
    cm = lambda a: torch.from_numpy(a).cuda().t().contiguous().t()
    kw = dict(dt=SR.MONTH, theta=0.5, nsteps=3, first_slot=1, rtol=RTOL, maxiter=MAXITER, precond="lines")
    Xa, ia = asm.step_tracers(cm(X0), observe=cm(W), time_weights=tw, **kw)
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, *months[0])) as D:
        D.set_lines(asm.vertical_lines().cpu().numpy())
        D.set_slots(2)
        D.set_values(months[1][2], slot=1)
        Xo, io = D.step(X0, observe=W, time_weights=tw, **kw)
    assert ia.steps_done == io.steps_done == 3
    _same_bits(Xa.cpu().numpy(), Xo, "X")
    _same_bits(ia.observations.cpu().numpy(), io.observations, "observations")
    _same_bits(ia.mean.cpu().numpy(), io.mean, "mean")


def test_the_inventory_is_conserved_within_the_solvers_stop_rule(oracle):
    """A test of use.  On tiny_tripolar the oracle's T has vᵀ·T = 0 for v the cell volumes (to rounding: max |vᵀ·T| is 1.6e-16 of
    |v|ᵀ·|T|), not 1ᵀ·T = 0 (3e-4 against 1e-3), so the observer is v: the inventory.  θ = 1, no source, no d, slots T, T/2, T/4 (exact scalings
    keep the null vector): (σ·I + A)·x⁺ = σ·x - r with ‖r‖₂ <= rtol·‖b‖₂ by the solver's stop rule, hence vᵀ·x⁺ - vᵀ·x = -vᵀ·r / σ and
    |change| <= ‖v‖₂·rtol·‖b‖₂/σ, plus what the two observations themselves may be off: roundings·2⁻⁵³·Σ|v·x| each.  Nothing is tuned."""
    import otmb_amd.api as api
    from helpers import make_case

    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    p, i, v = T
    gm = make_case("tiny_tripolar")[1]
    idx = oracle.makeindices(gm.v3D)
    wet = np.asarray(idx["wet3D"]).astype(bool)
    vol = np.zeros(N)
    vol[np.asarray(idx["Lwet3D"])[wet] - 1] = np.asarray(gm.v3D)[wet]
    A = R.csc_of(N, N, p, i, v)
    assert np.abs(A.T @ vol).max() <= 1e-14 * (abs(A).T @ vol).max()  # the volumes are the left null vector ...
    assert np.abs(A.T @ np.ones(N)).max() >= 1e-2 * (abs(A).T @ np.ones(N)).max()  # ... and the ones vector is not
    sigma = SR.constants(SR.MONTH, 1.0)[0]
    X0 = _start(N, K, 47)
    nsteps = 6
    with api.DeviceOperator(_csc(N, p, i, v)) as D:
        D.set_slots(3)
        D.set_values(0.5 * v, slot=1)
        D.set_values(0.25 * v, slot=2)
        D.set_lines(nxt)
        X, info = D.step(X0, dt=SR.MONTH, theta=1.0, nsteps=nsteps, first_slot=0, observe=vol, rtol=RTOL, maxiter=MAXITER, precond="lines")
        states = [X0] + _chain(D, X0, nsteps, 0, dt=SR.MONTH, theta=1.0, rtol=RTOL, maxiter=MAXITER, precond="lines")
        first = D.observe(vol, X0)[0]
    assert info.status == 0 and info.steps_done == nsteps
    inv = np.concatenate([first[None, :], info.observations[:, :, 0]])  # (nsteps + 1, k)
    for t in range(nsteps):
        for c in range(K):
            solver = np.linalg.norm(vol) * RTOL * np.linalg.norm(sigma * states[t][:, c]) / sigma
            rounding = OR.roundings(N) * 2.0 ** -53 * (math.fsum(np.abs(vol * states[t][:, c])) + math.fsum(np.abs(vol * states[t + 1][:, c])))
            change = abs(inv[t + 1, c] - inv[t, c])
            print("step", t, "column", c, "inventory", inv[t + 1, c], "change", change, "solver's bound", solver, "rounding", rounding)
            assert change <= solver + rounding, (t, c)
