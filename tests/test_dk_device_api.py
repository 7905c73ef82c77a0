"""GPU: device.Operator with a 2-D d (a torch tensor with its own leading dimension) in step, step with observers and the mean's weights,
and periodic with outer none and mean: the bits of api.DeviceOperator's call on the same matrix, slots and lines.  The observations and the
mean of a per-column step are also judged by tests/observe_ref.py on the states that the per-column step itself returns after 1, 2, ...
steps: the restatement shares no code with the library's observation pass.  The shape refusals of device.Operator, and the singular
preconditioner's message of a per-column step and of a per-column periodic call, which names the caller's column and k although the periodic
driver hands the step a gathered block without the zero-source columns (and, with a start, every column twice)."""
import re

import numpy as np
import pytest

import dk_cases as DK
import observe_ref as OR
import solve_lines_ref as LR
import solve_ref as R
from test_op_padded_dev import _pad, _same, _System
from test_step import _operator

pytestmark = pytest.mark.gpu

N0, K, Q = 257, DK.K, 3
NSTEPS, FIRST, DT = 4, 2, 2.0
RTOL, MAXITER = 1e-10, 5000


def _cm(a):
    """A host array as a column-major device tensor."""
    import torch

    a = np.asarray(a, dtype=np.float64)
    return torch.from_numpy(a.copy()).cuda() if a.ndim == 1 else torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


@pytest.fixture(scope="module")
def both():
    """dominant (n = 257) with the tests' three slots and random lines, as a device.Operator and as an api.DeviceOperator; D (one zero
    column), its device copy at ldd = n + 3 with NaN below row n, a start, a source, observers and weights."""
    from otmb_amd.device import DeviceAssembler

    nxt = LR.random_lines(N0, 3)
    P = _System(DeviceAssembler(0).ctx, N0, R.dominant(N0), None, 0.5, K, nxt=nxt)
    H = _operator(N0, *R.dominant(N0), nxt=nxt)
    rng = np.random.default_rng(71)
    D = np.asfortranarray(rng.uniform(0.0, 1.0, (N0, K)) * np.array([1.0, 1e-3, 10.0, 0.0, 5.0, 0.3, 2.0]))
    X0, S = DK.rhs(N0, K, seed=72), np.asfortranarray(rng.standard_normal((N0, K)))
    W, tw = np.asfortranarray(rng.uniform(0.0, 1.0, (N0, Q))), rng.uniform(0.0, 1.0, NSTEPS)
    yield P.O, H, D, _pad(D, 3, np.nan)[:N0], X0, S, W, tw
    P.O.close()
    H.close()


@pytest.mark.parametrize("theta,adjoint,precond", [(1.0, False, "jacobi"), (0.5, True, "lines"), (0.5, False, "lines")])
def test_step_on_device_tensors_is_the_host_call(both, theta, adjoint, precond):
    O, H, D, Dt, X0, S, W, tw = both
    assert Dt.stride() == (1, N0 + 3)
    kw = dict(dt=DT, theta=theta, nsteps=NSTEPS, first_slot=FIRST, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
    for source in (None, S):
        Xh, ih = H.step(X0, d=D, source=source, **kw)
        Xd, idev = O.step(_cm(X0), d=Dt, source=None if source is None else _cm(source), **kw)
        assert ih.status == 0 and idev.status == 0 and idev.steps_done == NSTEPS == ih.steps_done
        _same(Xd, Xh, ("state", source is not None))
        assert np.array_equal(idev.iterations, ih.iterations) and idev.reason == ih.reason
        _same(idev.relres, ih.relres, "relres")
        assert idev.observations is None and idev.mean is None
    assert len(set(ih.iterations[0].tolist())) > 1, ih.iterations  # the columns are different systems
    # observers and the mean's weights, together and each alone
    states = [H.step(X0, d=D, source=S, **dict(kw, nsteps=t + 1))[0] for t in range(NSTEPS)]
    _same(states[-1], Xh, "the state after t + 1 steps is the longer call's")
    want_obs = np.stack([OR.observe_ref(W, X).T for X in states])  # (nsteps, k, q)
    want_mean = OR.mean_ref(states, tw)
    for observe, weights in ((W, tw), (W, None), (None, tw)):
        Xh2, ih2 = H.step(X0, d=D, source=S, observe=observe, time_weights=weights, **kw)
        Xd2, id2 = O.step(_cm(X0), d=Dt, source=_cm(S), observe=None if observe is None else _cm(observe), time_weights=weights, **kw)
        _same(Xh2, Xh, "the observers change nothing of the state")
        _same(Xd2, Xh, "device state with observers")
        assert np.array_equal(id2.iterations, ih.iterations)
        for info, where in ((ih2, "host"), (id2, "device")):
            assert (info.observations is None) == (observe is None) and (info.mean is None) == (weights is None)
            if observe is not None:
                _same(info.observations, want_obs, (where, "observations against observe_ref"))
            if weights is not None:
                _same(info.mean, want_mean, (where, "mean against observe_ref's fold"))
    # a 1-D state with its 2-D d has no column to pair with; k = 1 as a matrix has
    x1, i1 = O.step(_cm(X0[:, 2:3]), d=Dt[:, 2:3], source=_cm(S[:, 2:3]), **kw)
    _same(x1, Xh[:, 2:3], "k = 1 as a matrix")


@pytest.mark.parametrize("outer", ["none", "mean"])
def test_periodic_on_device_tensors_is_the_host_call(both, outer):
    O, H, D, Dt, X0, S, W, tw = both
    kw = dict(dt=DT, ncycle=4, theta=0.5, first_slot=FIRST, rtol=1e-12, maxiter=MAXITER, precond="lines", ptol=1e-8, restart=7, maxcycles=200, outer=outer)
    for x0 in (None, X0):
        Xh, ih = H.periodic(S, d=D, x0=x0, **kw)
        Xd, idev = O.periodic(_cm(S), d=Dt, x0=None if x0 is None else _cm(x0), **kw)
        print(outer, x0 is not None, "cycles", ih.cycles.tolist(), "mean-solve iterations", ih.msolve_iters.tolist())
        assert ih.status == 0 and idev.status == 0 and ih.converged.all()
        _same(Xd, Xh, (outer, "X"))
        assert np.array_equal(idev.cycles, ih.cycles) and np.array_equal(idev.msolve_iters, ih.msolve_iters) and np.array_equal(idev.reason, ih.reason)
        _same(idev.defect, ih.defect, "defect")
        assert (ih.msolve_iters > 0).all() == (outer == "mean")
    assert len(set(ih.cycles.tolist())) > 1, ih.cycles


def test_device_shapes_are_refused(both):
    import torch

    from otmb_amd import capi

    O, H, D, Dt, X0, S, W, tw = both
    X, x = _cm(X0), _cm(X0[:, 0])
    cases = [(x, Dt, r"DimensionMismatch: d of \(257, 7\) is per column, \w+ of \(257,\) has no columns"),
             (X, Dt[:, :K - 1], r"DimensionMismatch: d must be float64 of \w+'s shape \(257, 7\), not \(257, 6\)"),
             (X, Dt[:N0 - 1], r"DimensionMismatch: d must be float64 of \w+'s shape \(257, 7\), not \(256, 7\)"),
             (X, Dt.to(torch.float32), r"DimensionMismatch: d must be float64 of \w+'s shape \(257, 7\), not \(257, 7\)")]
    for B, d, pattern in cases:
        for call in (lambda: O.solve(B, d=d), lambda: O.precondition(B, d=d, precond="jacobi"), lambda: O.step(B, d=d, dt=DT),
                     lambda: O.step(B, d=d, dt=DT, time_weights=np.ones(1)), lambda: O.periodic(B, d=d, dt=DT, ncycle=2),
                     lambda: O.periodic(B, d=d, dt=DT, ncycle=2, outer="mean")):
            with pytest.raises(capi.OtmbError) as err:
                call()
            assert err.value.status == 11 and re.fullmatch(pattern, str(err.value)), str(err.value)


def test_the_singular_message_of_step_and_periodic_names_the_callers_column(both):
    """Column 3 of D makes the step's diagonal non-finite at one index, column 6 at a smaller one: a per-column step names column 3 of 7 and
    that index.  In periodic, column 1 has no source, so the step call holds columns 2 to 7 (and, with a start, each of them twice): the
    message still names column 3 of 7.  Nothing is written: the calls return no state."""
    from otmb_amd import capi

    O, H, D, Dt, X0, S, W, tw = both
    bad = D.copy(order="F")
    bad[40, 2] = np.inf
    bad[7, 5] = np.inf
    Sz = S.copy(order="F")
    Sz[:, 0] = 0.0
    text = "diag(M)[41] is zero or not finite (1-based; the first such index) (column 3 of 7)"
    with pytest.raises(capi.OtmbError) as err:
        H.step(X0, d=bad, dt=DT, first_slot=FIRST, precond="jacobi")
    assert err.value.name == "SINGULAR_PRECONDITIONER" and text in str(err.value), str(err.value)
    for x0 in (None, X0):
        for outer in ("none",) if x0 is not None else ("none", "mean"):
            with pytest.raises(capi.OtmbError) as err:
                H.periodic(Sz, d=bad, x0=x0, dt=DT, ncycle=4, first_slot=FIRST, precond="jacobi", outer=outer)
            assert err.value.name == "SINGULAR_PRECONDITIONER" and text in str(err.value), (outer, str(err.value))
    Xh, ih = H.periodic(Sz, d=D, dt=DT, ncycle=4, theta=0.5, first_slot=FIRST, rtol=1e-12, maxiter=MAXITER, precond="lines", restart=7, maxcycles=200,
                        outer="mean")
    assert ih.status == 0 and (Xh[:, 0] == 0.0).all()  # the operator is still usable, and the zero-source column is answered with zero
