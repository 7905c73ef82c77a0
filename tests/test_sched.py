"""GPU: otmb_op_step_sched (csrc/otmb_step.hip): θ-steps with a schedule -- several sub-steps inside a slot, a source per slot, a factor per
step and tracer on the source.  The contract of include/otmb.h in public calls: step t of a scheduled call has the bits of the ONE-step
step() with first_slot = slot(t) and the source S_j·scale[t] formed in numpy, from the state step t - 1 left -- states, steps_done,
iterations, relres, reasons; a scale of ones is no scale; a column of seven is the column alone; the record (observations, mean) is that
of the chain's states; refusals leave everything as it was; a step that fails names its step and the schedule's slot; and separate,
padded, misaligned device tensors give the compact call's bits."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dk_cases as DK
import observe_ref as OR
import sched_ref as SC
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _csc, _operator, _start

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
NSTEPS, FIRST, NSLOTS = 8, 2, 3


def _scale(nsteps, k, seed=5):
    """A seeded history with a 0.0, a negative value and a 1.0 in every column."""
    f = np.random.default_rng(seed).uniform(0.25, 2.0, (nsteps, k))
    for c in range(k):
        f[(c + 1) % nsteps, c], f[(c + 2) % nsteps, c], f[(c + 3) % nsteps, c] = 0.0, -1.5, 1.0
    return f


def _sources(N, k, nsrc, seed, size=1e-7):
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(rng.standard_normal((N, k)) * size) for _ in range(nsrc)]


def _chain(D, X0, *, nsteps, first_slot, substeps, source, scale, **kw):
    """The contract in public calls: one-step step() calls with S_eff formed in numpy.  -> (X, steps_done, rows, the states after every step)"""
    X, done, rows, states = np.array(X0, order="F"), 0, [], []
    for t in range(nsteps):
        slot = SC.slot_of(t, first_slot, substeps, NSLOTS)
        X, info = D.step(X, nsteps=1, first_slot=slot, source=SC.s_eff(source, scale, t, slot), **kw)
        rows.append((info.iterations[0], info.relres[0], info.reason[0]))
        if info.steps_done != 1:
            break
        done = t + 1
        states.append(X)
    return X, done, rows, states


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117), the tests' three slots and the water columns; the age d and the seven-column D; a start, three source blocks of
    seven columns and a history of 8 x 7."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    D = _operator(N, *T, nxt=nxt)
    yield D, N, R.shift("age", N, nsurf)[0], DK.columns(N, nsurf, zero=True), _start(N, 7, 12), _sources(N, 7, 3, 11), _scale(NSTEPS, 7)
    D.close()


# (nsrc, a scale, d): with every (k, substeps) three of these six, alternately the even and the odd ones -- every value of each meets every k
# and every substeps, at a fraction of the cross product's 12
COMBOS = [(1, False, "none"), (3, True, "age"), (1, True, "D"), (3, False, "D"), (3, True, "none"), (1, False, "age")]


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_scheduled_step_has_the_bits_of_the_chain_of_single_steps(small, theta, adjoint, precond):
    """N = 117, 8 steps from slot 2 of 3: k = 1, 3, 7 (register blocks 1; 2 + 1; 4 + 2 + 1: the scale's offset c0 is 0, 2, 4, 6) x substeps 1, 2
    (slot 2 comes back after the wrap: its kept preconditioner), 3 (the last run is partial) x one source or three x no scale or one with a
    0.0, a negative value and a 1.0 x no d, the age d, a D of its own per column."""
    D, N, dage, Dk, X7, S7, F7 = small
    for idx, (k, m) in enumerate(itertools.product((1, 3, 7), (1, 2, 3))):
        for nsrc, scaled, dkind in COMBOS[idx % 2::2]:
            if dkind == "D" and k == 1:
                dkind = "age"  # (a 1-D state has no per-column d)
            X0 = X7[:, 0] if k == 1 else X7[:, :k]
            src = [S[:, 0] if k == 1 else S[:, :k] for S in S7[:nsrc]]
            scale = None if not scaled else F7[:, 0] if k == 1 else np.ascontiguousarray(F7[:, :k])
            d = {"none": None, "age": dage, "D": np.asfortranarray(Dk[:, :k])}[dkind]
            kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, substeps=m, source=src, scale=scale, d=d, rtol=RTOL, maxiter=MAXITER,
                      adjoint=adjoint, precond=precond)
            sched = dict(kw, source_scale=kw["scale"])
            del sched["scale"]
            what = (theta, adjoint, precond, k, m, nsrc, scaled, dkind)
            Xs, info = D.step_sched(X0, **sched)
            chain = {key: kw[key] for key in kw if key != "substeps"}
            Xc, done, rows, _ = _chain(D, X0, substeps=m, **chain)
            assert info.status == 0 and info.steps_done == done == NSTEPS, (what, info)
            DK.same_bits(Xs, Xc, (what, "state"))
            for t, (it, rr, why) in enumerate(rows):
                assert np.array_equal(info.iterations[t], it) and info.reason[t] == why, (what, t)
                DK.same_bits(info.relres[t], rr, (what, t, "relres"))
    assert D.slots == (NSLOTS, 0)  # the selection is the caller's


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_a_scale_of_ones_and_a_column_alone(small, theta, precond):
    """k = 7, substeps = 2, three sources, the per-column D: a scale of all 1.0 has the bits of no scale; columns 0, 3 and 6 (the first of
    the block of four, its last, the block of one) have the bits of the column stepped alone with its own column of every block, of the
    scale and of D -- and differ from each other."""
    D, N, dage, Dk, X7, S7, F7 = small
    kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, substeps=2, d=Dk, rtol=RTOL, maxiter=MAXITER, precond=precond)
    Xn, i_n = D.step_sched(X7, source=S7, **kw)
    X1, i_1 = D.step_sched(X7, source=S7, source_scale=np.ones((NSTEPS, 7)), **kw)
    DK.same_bits(Xn, X1, "a scale of ones")
    assert np.array_equal(i_n.iterations, i_1.iterations) and i_n.steps_done == i_1.steps_done == NSTEPS
    DK.same_bits(i_n.relres, i_1.relres, "a scale of ones: relres")
    Xs, info = D.step_sched(X7, source=S7, source_scale=F7, **kw)
    assert not np.array_equal(Xs, Xn)
    for c in (0, 3, 6):
        xc, ic = D.step_sched(X7[:, c], source=[S[:, c] for S in S7], source_scale=np.ascontiguousarray(F7[:, c]),
                              **dict(kw, d=np.ascontiguousarray(Dk[:, c])))
        DK.same_bits(xc, Xs[:, c], ("column alone", c))
        assert np.array_equal(ic.iterations[:, 0], info.iterations[:, c]) and ic.steps_done == NSTEPS
        DK.same_bits(ic.relres[:, 0], info.relres[:, c], ("column alone: relres", c))
    # one source for every step, given as an array: the same call as the list of one
    Xa, _ = D.step_sched(X7, source=S7[1], source_scale=F7, **kw)
    Xl, _ = D.step_sched(X7, source=[S7[1]], source_scale=F7, **kw)
    DK.same_bits(Xa, Xl, "an array is a list of one")


@pytest.mark.parametrize("name", ["tiny_tripolar", "small_rho3d"])
def test_larger_grids(oracle, name):
    """N = 429 and 6962 (several workgroups and slices): k = 7, lines, substeps = 2, three sources, a scale, the age d; θ = 0.5 with A and Aᵀ,
    θ = 1 with A; 5 steps from slot 2 (2, 2, 0, 0, 1)."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    d = R.shift("age", N, nsurf)[0]
    S, F, X0 = _sources(N, 7, 3, 21), _scale(5, 7), _start(N, 7, 22)
    with _operator(N, *T, nxt=nxt) as D:
        for theta, adjoint in ((0.5, False), (0.5, True), (1.0, False)):
            kw = dict(dt=SR.MONTH, theta=theta, nsteps=5, first_slot=FIRST, substeps=2, source=S, d=d, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                      precond="lines")
            Xs, info = D.step_sched(X0, source_scale=F, **kw)
            Xc, done, rows, _ = _chain(D, X0, scale=F, **kw)
            assert info.status == 0 and info.steps_done == done == 5, (name, theta, adjoint, info)
            DK.same_bits(Xs, Xc, (name, theta, adjoint))
            assert np.array_equal(info.iterations, np.array([r[0] for r in rows]))
            DK.same_bits(info.relres, np.array([r[1] for r in rows]), (name, theta, adjoint, "relres"))


@pytest.mark.parametrize("adjoint", [False, True])
def test_a_long_row(adjoint):
    """solve_ref.arrow(5000): the long-row workgroup of the right-hand side's kernel, where the lane is the tracer and reads f[lane];
    θ = 0.5, k = 3, three sources, a scale."""
    n = 5000
    p, i, v = R.arrow(n)
    S, F = _sources(n, 3, 3, 31, size=1.0), _scale(5, 3)
    with _operator(n, p, i, v) as D:
        kw = dict(dt=SR.MONTH, theta=0.5, nsteps=5, first_slot=FIRST, substeps=2, source=S, d=None, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                  precond="jacobi")
        Xs, info = D.step_sched(_start(n, 3, 32), source_scale=F, **kw)
        Xc, done, rows, _ = _chain(D, _start(n, 3, 32), scale=F, **kw)
        assert info.status == 0 and info.steps_done == done == 5
        DK.same_bits(Xs, Xc, ("arrow", adjoint))
        assert np.array_equal(info.iterations, np.array([r[0] for r in rows]))


def test_the_record_under_a_schedule(small):
    """observe and time_weights: the observations are observe() of the chain's states, the mean is observe_ref.mean_ref of them, and X and
    the report are the plain scheduled call's."""
    D, N, dage, Dk, X7, S7, F7 = small
    rng = np.random.default_rng(71)
    W, tw = np.asfortranarray(rng.uniform(0.0, 1.0, (N, 3))), rng.uniform(0.0, 1.0, NSTEPS)
    X0, S, F = X7[:, :3], [s[:, :3] for s in S7], np.ascontiguousarray(F7[:, :3])
    for theta, adjoint in ((1.0, False), (0.5, True)):
        kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, substeps=3, source=S, d=dage, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                  precond="lines")
        Xp, ip = D.step_sched(X0, source_scale=F, **kw)
        Xr, ir = D.step_sched(X0, source_scale=F, observe=W, time_weights=tw, **kw)
        _, done, _, states = _chain(D, X0, scale=F, **kw)
        assert ip.observations is None and ip.mean is None and done == NSTEPS
        DK.same_bits(Xr, Xp, "X with a record")
        assert np.array_equal(ir.iterations, ip.iterations) and ir.steps_done == NSTEPS
        DK.same_bits(ir.relres, ip.relres, "relres with a record")
        assert ir.observations.shape == (NSTEPS, 3, 3)
        for t, Xt in enumerate(states):
            DK.same_bits(ir.observations[t], D.observe(W, Xt).T, ("observations", t))
        DK.same_bits(ir.mean, OR.mean_ref(states, tw), "the mean")


def _sched_c(D, X, ldx, k, *, nsteps=4, first_slot=0, substeps=1, S=(), nsrc=None, lds=None, scale=None, dt=SR.MONTH, theta=1.0, rtol=RTOL,
             maxiter=MAXITER, precond=0, dev=False):
    """otmb_op_step_sched through the C ABI; S: a sequence of arrays or None (a null block), or None (a null array).
    -> (status, steps_done, iters) with the report preset to sentinels."""
    from otmb_amd import capi

    it, rr, why = np.full((max(nsteps, 1), k), -7, np.int64), np.full((max(nsteps, 1), k), 7.25), np.full((max(nsteps, 1), k), -7, np.int32)
    done = C.c_int64(-7)
    arr = None if S is None else (C.c_void_p * max(len(S), 1))(*[None if s is None else s.ctypes.data for s in S])
    rc = capi.lib().otmb_op_step_sched(D.handle, 0, k, None, 0, float(dt), float(theta), nsteps, first_slot, substeps, len(S) if nsrc is None else nsrc, arr,
                                       (X.shape[0] if lds is None else lds), None if scale is None else scale.ctypes.data, X.ctypes.data, ldx, float(rtol),
                                       maxiter, precond, C.byref(done), it.ctypes.data, rr.ctypes.data, why.ctypes.data, 0, None, 0, None, None, None, 0)
    return rc, done.value, it


def test_refusals_leave_x_and_the_operator_unchanged(small):
    from otmb_amd import capi

    D, N, dage, Dk, X7, S7, F7 = small
    X0 = np.asfortranarray(X7[:, :2])
    S3 = [np.asfortranarray(s[:, :2]) for s in S7]
    before = D.mul(X0)
    nan, inf = np.ones((4, 2)), np.ones((4, 2))
    nan[2, 1], inf[3, 0] = np.nan, np.inf
    bad = [(dict(substeps=0), "substeps must be >= 1"), (dict(substeps=-3, S=S3), "substeps must be >= 1"),
           (dict(S=S3[:2]), "nsrc must be 0, 1 or the number of slots"), (dict(S=S3 + S3[:1]), "nsrc must be 0, 1 or the number of slots"),
           (dict(nsrc=-1), "nsrc must be 0, 1 or the number of slots"),
           (dict(S=None, nsrc=1), "S is null with nsrc > 0"), (dict(S=None, nsrc=3), "S is null with nsrc > 0"),
           (dict(S=[S3[0], None, S3[2]]), "a source block is null"),
           (dict(S=S3, lds=N - 1), None),  # (refused by the checks of the call it extends: the first block's lds)
           (dict(scale=np.ones((4, 2))), "scale needs a source (nsrc > 0)"),
           (dict(S=S3, scale=nan), "a scale value is not finite"), (dict(S=S3[:1], scale=inf), "a scale value is not finite")]
    for kw, text in bad:
        X = X0.copy(order="F")
        rc, done, it = _sched_c(D, X, N, 2, **kw)
        msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
        assert rc == 11, (kw.keys(), rc, msg)
        assert np.array_equal(X, X0) and (it == -7).all() and D.slots == (NSLOTS, 0), kw.keys()
        if text is not None:
            assert msg == f"{capi.lib().otmb_status_string(11).decode()}: otmb_op_step_sched: {text}", msg
    # ... after the checks of the call they extend: with two bad arguments the older complaint comes first
    X = X0.copy(order="F")
    assert _sched_c(D, X, N, 2, substeps=0, dt=0.0)[0] == 11
    assert capi.lib().otmb_last_error(D.ctx.handle).decode().endswith("dt must be > 0 and finite")
    # the Python layer raises them
    for kw in (dict(substeps=0), dict(source=S3, source_scale=nan)):
        with pytest.raises(capi.OtmbError) as e:
            D.step_sched(X0, dt=SR.MONTH, nsteps=4, **kw)
        assert e.value.name == "INVALID_ARG" and "otmb_op_step_sched" in str(e.value)
    DK.same_bits(D.mul(X0), before, "the operator after the refusals")
    # and a call that is in order still runs, through the same handle
    X = X0.copy(order="F")
    rc, done, it = _sched_c(D, X, N, 2, S=S3, substeps=2, scale=np.ones((4, 2)))
    want, _ = D.step_sched(X0, dt=SR.MONTH, nsteps=4, substeps=2, source=S3)
    assert rc == 0 and done == 4
    DK.same_bits(X, want, "the C call after the refusals")


def test_a_step_that_does_not_converge_names_its_step_and_the_schedules_slot(oracle):
    """Slot 0 holds 1e-6·T (a handful of Jacobi iterations a step), slot 1 holds T (about 190): with maxiter = 20 and two sub-steps a slot the
    call completes steps 0 and 1 in slot 0 and ends at step 2, the first in slot 1."""
    import otmb_amd.api as api
    from otmb_amd import capi

    T, N, _, _ = LR.grid(oracle, "odd_nx_fold")
    X0, S = _start(N, 2, 71), _sources(N, 2, 2, 72)
    with api.DeviceOperator(_csc(N, T[0], T[1], 1e-6 * T[2])) as E:
        E.set_slots(2)
        E.set_values(T[2], slot=1)
        Xs, info = E.step_sched(X0, dt=SR.MONTH, nsteps=6, substeps=2, source=S, rtol=RTOL, maxiter=20)
        msg = capi.lib().otmb_last_error(E.ctx.handle).decode()
        print(info, msg)
        assert info.status == capi.NOT_CONVERGED and info.steps_done == 2 and len(info.iterations) == 3
        assert info.converged[:2].all() and "maxiter" in info.reason[2]
        assert msg.endswith("(step 2, slot 1)"), msg
        X, done = np.array(X0, order="F"), 0
        for t in range(3):  # the chain's last iterates
            X, one = E.step(X, dt=SR.MONTH, nsteps=1, first_slot=t // 2, source=S[t // 2], rtol=RTOL, maxiter=20)
        assert one.steps_done == 0
        DK.same_bits(Xs, X, "the failing step's last iterates")
        assert E.slots == (2, 0)


def test_the_device_route_with_separate_padded_misaligned_sources():
    """device.Operator.step_sched at n = 4609: the three source blocks are separate tensors, each with a padded leading dimension and a base
    8 bytes off a 16-byte boundary; the result has the bits of the call on compact tensors (θ = 0.5 with Aᵀ, θ = 1 with A), and at θ = 1 of
    the host route."""
    import torch

    from otmb_amd import device

    n, k, nsteps = 4609, 3, 3  # (slots 2, 2, 0: the solves at this n take most of a second a step, so three steps and two cases)
    p, i, v = R.dominant(n)
    dev = torch.device("cuda", 0)
    ctx = device.DeviceAssembler(0).ctx
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    X0, S, F = _start(n, k, 81), _sources(n, k, 3, 82, size=1.0), _scale(nsteps, k)
    d = np.random.default_rng(83).uniform(0.0, 1.0, n)

    def padded(a, pad=5):
        ld = n + pad
        buf = torch.full((1 + ld * k,), float("nan"), dtype=torch.float64, device=dev)
        view = buf[1:].as_strided((n, k), (1, ld))
        view.copy_(t(a.T, np.float64).t())
        assert view.data_ptr() % 16 == 8
        return view

    nxt = LR.random_lines(n, 3)
    with _operator(n, p, i, v, nxt=nxt) as D, device.Operator(ctx, n, n, t(p, np.int64), t(i, np.int64), t(v, np.float64)) as O:
        O.set_slots(3)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            O.set_values_dev(t(vals, np.float64), slot=s)
        O.set_lines(t(nxt, np.int64))
        Xd = t(X0.T, np.float64).t()
        compact, pads = [t(s.T, np.float64).t() for s in S], [padded(s) for s in S]
        for theta, adjoint, precond in ((0.5, True, "lines"), (1.0, False, "lines")):
            kw = dict(dt=2.0, theta=theta, nsteps=nsteps, first_slot=FIRST, substeps=2, source_scale=F, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                      precond=precond)
            Xc, ic = O.step_sched(Xd, source=compact, d=t(d, np.float64), **kw)
            Xp, ip = O.step_sched(Xd, source=pads, d=t(d, np.float64), **kw)
            assert ic.steps_done == ip.steps_done == nsteps
            DK.same_bits(Xp.cpu().numpy(), Xc.cpu().numpy(), ("padded and misaligned", theta, adjoint, precond))
            assert np.array_equal(ip.iterations, ic.iterations)
            if theta == 1.0:
                Xh, ih = D.step_sched(X0, source=S, d=d, **kw)
                DK.same_bits(Xc.cpu().numpy(), Xh, ("device route against the host route", theta, adjoint, precond))
                assert ih.steps_done == nsteps and np.array_equal(ic.iterations, ih.iterations)
        assert O.slots == (3, 0)
