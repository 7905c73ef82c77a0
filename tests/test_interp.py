"""GPU: otmb_op_step_interp (csrc/otmb_step.hip, csrc/otmb_interp.hip): θ-steps whose matrix is interpolated between two value slots.  The
contract of include/otmb.h in PUBLIC calls on the same operator, which has one slot more than the cycle as the chain's scratch: a plain
step (a == b, w == 0.0, w == 1.0) has the bits of the one-step step() on its slot; a blended step those of combine_slots() with 1.0 - w at
a, w at b and zero elsewhere into the scratch slot, followed by the one-step step() on it -- states, steps_done, iterations, relres,
reasons; a column of seven is the column alone; the record is that of the chain's states; refusals leave everything as it was; a failure
names its step, both slots and the weight; separate, padded, misaligned device tensors give the compact call's bits.

Why this covers the blend kernel: it writes two arrays, `val` of the row layout and `nz` of the CSC copy.  The product A·X reads val; the
product Aᵀ·X and both preconditioners (Jacobi's diagonal, the lines' extraction) read nz.  So θ = 0.5 -- whose right-hand side holds the
product -- with both values of adjoint makes every blended entry of both arrays count in the compared bits, at array lengths below one
chunk of the kernel (odd_nx_fold), between one and two (tiny_bipolar) and far beyond two (90x60x20), with odd and even nnz."""
import ctypes as C

import numpy as np
import pytest

import dk_cases as DK
import interp_ref as IR
import observe_ref as OR
import sched_ref as SC
import solve_lines_ref as LR
import solve_ref as R
import spmv_edges as E
import step_ref as SR
from test_step import _csc, _start

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
NSLOTS, SPARE = 3, 3  # the cycle's slots 0 .. 2 and the chain's scratch slot
IP_SPAN = 2048        # csrc/otmb_interp.hip: entries per chunk of the blend kernel

# step:     0 plain (a == b)   1 blend   2 plain (w == 0.0) on 1   3 blend, the wrap pair   4 the same pair again   5 plain (w == 1.0) on 2
#           6 blend, w = 1/3   7 plain on 0 again: the preconditioner kept since step 0
HAND = (np.array([0, 0, 1, 2, 2, 1, 0, 0]), np.array([0, 1, 2, 0, 0, 2, 2, 1]), np.array([0.7, 0.25, 0.0, 0.5, 0.5, 1.0, 1.0 / 3.0, 0.0]))
NSTEPS = 8


def _operator(n, p, i, v, nxt=None):
    """A DeviceOperator with the tests' three slots (step_ref.slot_values) and a fourth as the chain's scratch, and optionally lines."""
    import otmb_amd.api as api

    D = api.DeviceOperator(_csc(n, p, i, v))
    D.set_slots(NSLOTS + 1)
    for s, vals in enumerate(SR.slot_values(v, seed=1)):
        D.set_values(vals, slot=s)
    if nxt is not None:
        D.set_lines(nxt)
    return D


def _lengths(n, p, i):
    """(nnz, nval): the entries of the two value arrays the blend kernel writes (nval from the mirror of the row layout, tests/spmv_edges.py)."""
    L = E.layout(n, n, p, i)
    return int(p[-1] - 1), int(64 * L.width.sum() + L.lens[L.long].sum())


def _sources(N, k, seed, size=1e-7):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal((N, k)) * size)


def _scale(nsteps, k, seed=5):
    f = np.random.default_rng(seed).uniform(0.25, 2.0, (nsteps, k))
    for c in range(k):
        f[(c + 1) % nsteps, c], f[(c + 2) % nsteps, c], f[(c + 3) % nsteps, c] = 0.0, -1.5, 1.0
    return f


def _chain(D, X0, sched, *, source, scale, **kw):
    """The contract in public calls.  -> (X, steps_done, rows, the states after every completed step)"""
    X, done, rows, states = np.array(X0, order="F"), 0, [], []
    for t, (a, b, w) in enumerate(zip(*sched)):
        what, slot = IR.kind(int(a), int(b), float(w))
        if what == "blend":
            D.combine_slots(IR.combine_weights(NSLOTS + 1, int(a), int(b), float(w)), SPARE)
            slot = SPARE
        X, info = D.step(X, nsteps=1, first_slot=slot, source=SC.s_eff(None if source is None else [source], scale, t, 0), **kw)
        rows.append((info.iterations[0], info.relres[0], info.reason[0]))
        if info.steps_done != 1:
            break
        done = t + 1
        states.append(X)
    return X, done, rows, states


def _same_as_the_chain(D, X0, sched, what, *, source=None, scale=None, **kw):
    Xs, info = D.step_interp(X0, slot_a=sched[0], slot_b=sched[1], weight=sched[2], source=source, source_scale=scale, **kw)
    Xc, done, rows, states = _chain(D, X0, sched, source=source, scale=scale, **kw)
    nsteps = len(sched[2])
    assert info.status == 0 and info.steps_done == done == nsteps, (what, info)
    assert all(r == "converged" for row in info.reason for r in row), (what, info.reason)
    DK.same_bits(Xs, Xc, (what, "state"))
    for t, (it, rr, why) in enumerate(rows):
        assert np.array_equal(info.iterations[t], it) and info.reason[t] == why, (what, t)
        DK.same_bits(info.relres[t], rr, (what, t, "relres"))
    return Xs, info, states


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117, nnz = 681, odd; both value arrays below one chunk of the blend kernel), 3 + 1 slots and the water columns; the
    age d and the seven-column D; a start, a source of seven columns and a history of 8 x 7."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    nnz, nval = _lengths(N, T[0], T[1])
    assert nnz % 2 == 1 and 0 < nnz < IP_SPAN and 0 < nval < IP_SPAN, (nnz, nval)
    D = _operator(N, *T, nxt=nxt)
    yield D, N, R.shift("age", N, nsurf)[0], DK.columns(N, nsurf, zero=True), _start(N, 7, 12), _sources(N, 7, 11), _scale(NSTEPS, 7)
    D.close()


# (a source, a scale, d): with every k three of these six, alternately the even and the odd ones -- every value of each meets every k
COMBOS = [(False, False, "none"), (True, True, "age"), (True, False, "D"), (True, True, "D"), (False, False, "age"), (True, False, "none")]


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_interpolated_step_has_the_bits_of_the_chain_of_public_calls(small, theta, adjoint, precond):
    """N = 117, the hand-written eight steps (HAND): k = 1, 3, 7 (register blocks 1; 2 + 1; 4 + 2 + 1) x no source, a source, a source with a
    history x no d, the age d, a D of its own per column; and the convention's schedule interp_schedule(3, 2), six blended steps."""
    from otmb_amd import api

    D, N, dage, Dk, X7, S7, F7 = small
    for idx, k in enumerate((1, 3, 7)):
        for src, scaled, dkind in COMBOS[idx % 2::2]:
            if dkind == "D" and k == 1:
                dkind = "age"  # (a 1-D state has no per-column d)
            X0 = X7[:, 0] if k == 1 else X7[:, :k]
            S = None if not src else S7[:, 0] if k == 1 else S7[:, :k]
            scale = None if not scaled else F7[:, 0] if k == 1 else np.ascontiguousarray(F7[:, :k])
            d = {"none": None, "age": dage, "D": np.asfortranarray(Dk[:, :k])}[dkind]
            _same_as_the_chain(D, X0, HAND, (theta, adjoint, precond, k, src, scaled, dkind), source=S, scale=scale, dt=SR.MONTH, theta=theta, d=d, rtol=RTOL,
                               maxiter=MAXITER, adjoint=adjoint, precond=precond)
    tmm = api.interp_schedule(NSLOTS, 2)
    assert all(IR.kind(*s)[0] == "blend" for s in zip(*tmm)) and tuple(tmm[0]) == (2, 0, 0, 1, 1, 2)
    _same_as_the_chain(D, X7[:, :3], tmm, (theta, adjoint, precond, "TMM"), source=S7[:, :3], scale=None, dt=SR.MONTH / 2, theta=theta, d=dage, rtol=RTOL,
                       maxiter=MAXITER, adjoint=adjoint, precond=precond)
    assert D.slots == (NSLOTS + 1, 0)  # the selection is the caller's


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("name", ["tiny_bipolar", "90x60x20"])
def test_value_arrays_beyond_one_and_two_chunks(oracle, name, adjoint):
    """tiny_bipolar (N = 512): nnz = 3048, even, and nval both between one and two chunks of the blend kernel -- a full chunk and a partial one
    of each array.  90x60x20 (N = 65 817): nnz = 426 891, odd, and nval far beyond two chunks, so the row layout's array starts behind an odd
    count of CSC values and is indexed from its own base.  Two blended steps, k = 1, θ = 0.5, Jacobi."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    nnz, nval = _lengths(N, T[0], T[1])
    if name == "tiny_bipolar":
        assert nnz % 2 == 0 and IP_SPAN < nnz < 2 * IP_SPAN and IP_SPAN < nval < 2 * IP_SPAN, (nnz, nval)
    else:
        assert N == 65817 and nnz % 2 == 1 and nnz > 2 * IP_SPAN and nval > 2 * IP_SPAN, (nnz, nval)
    sched = (np.array([2, 0]), np.array([0, 1]), np.array([0.75, 1.0 / 3.0]))
    with _operator(N, *T) as D:
        _same_as_the_chain(D, _start(N, 1, 41)[:, 0], sched, (name, adjoint), source=_sources(N, 1, 42)[:, 0], dt=SR.MONTH, theta=0.5,
                           d=R.shift("age", N, nsurf)[0], rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="jacobi")
        assert D.slots == (NSLOTS + 1, 0)


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_a_column_alone_and_the_record(small, theta, precond):
    """k = 7 with the per-column D, a source and a history: columns 0, 3 and 6 (the first of the block of four, its last, the block of one)
    have the bits of the column stepped alone.  With observers and time weights, X and the report are the plain call's, the observations are
    observe() of the chain's states and the mean is observe_ref.mean_ref of them."""
    D, N, dage, Dk, X7, S7, F7 = small
    sched = dict(slot_a=HAND[0], slot_b=HAND[1], weight=HAND[2])
    kw = dict(dt=SR.MONTH, theta=theta, rtol=RTOL, maxiter=MAXITER, precond=precond, adjoint=theta == 0.5)
    Xs, info = D.step_interp(X7, source=S7, source_scale=F7, d=Dk, **sched, **kw)
    assert info.steps_done == NSTEPS
    for c in (0, 3, 6):
        xc, ic = D.step_interp(X7[:, c], source=S7[:, c], source_scale=np.ascontiguousarray(F7[:, c]), d=np.ascontiguousarray(Dk[:, c]), **sched, **kw)
        DK.same_bits(xc, Xs[:, c], ("column alone", c))
        assert np.array_equal(ic.iterations[:, 0], info.iterations[:, c]) and ic.steps_done == NSTEPS
        DK.same_bits(ic.relres[:, 0], info.relres[:, c], ("column alone: relres", c))
    assert not np.array_equal(Xs[:, 0], Xs[:, 3])
    rng = np.random.default_rng(71)
    W, tw = np.asfortranarray(rng.uniform(0.0, 1.0, (N, 3))), rng.uniform(0.0, 1.0, NSTEPS)
    X0, S, F = X7[:, :3], S7[:, :3], np.ascontiguousarray(F7[:, :3])
    Xp, ip = D.step_interp(X0, source=S, source_scale=F, d=dage, **sched, **kw)
    Xr, ir = D.step_interp(X0, source=S, source_scale=F, d=dage, observe=W, time_weights=tw, **sched, **kw)
    _, done, _, states = _chain(D, X0, HAND, source=S, scale=F, d=dage, **kw)
    assert ip.observations is None and ip.mean is None and done == NSTEPS
    DK.same_bits(Xr, Xp, "X with a record")
    assert np.array_equal(ir.iterations, ip.iterations) and ir.steps_done == NSTEPS
    DK.same_bits(ir.relres, ip.relres, "relres with a record")
    assert ir.observations.shape == (NSTEPS, 3, 3)
    for t, Xt in enumerate(states):
        DK.same_bits(ir.observations[t], D.observe(W, Xt).T, ("observations", t))
    DK.same_bits(ir.mean, OR.mean_ref(states, tw), "the mean")
    assert D.slots == (NSLOTS + 1, 0)


def _interp_c(D, X, ldx, k, a, b, w, *, S=(), nsrc=None, lds=None, scale=None, dt=SR.MONTH, theta=1.0, rtol=RTOL, maxiter=MAXITER, precond=0, nsteps=None):
    """otmb_op_step_interp through the C ABI; a, b, w: arrays or None (a null array); S: a sequence of arrays, or None (a null array).
    -> (status, steps_done, iters, reason) with the report preset to sentinels."""
    from otmb_amd import capi

    nsteps = max(len(x) for x in (a, b, w) if x is not None) if nsteps is None else nsteps
    it, rr, why = np.full((max(nsteps, 1), k), -7, np.int64), np.full((max(nsteps, 1), k), 7.25), np.full((max(nsteps, 1), k), -7, np.int32)
    done = C.c_int64(-7)
    a, b = (None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (a, b))
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    arr = None if S is None else (C.c_void_p * max(len(S), 1))(*[None if s is None else s.ctypes.data for s in S])
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = capi.lib().otmb_op_step_interp(D.handle, 0, k, None, 0, float(dt), float(theta), nsteps, ptr(a), ptr(b), ptr(w), len(S) if nsrc is None else nsrc, arr,
                                        (X.shape[0] if lds is None else lds), ptr(scale), X.ctypes.data, ldx, float(rtol), maxiter, precond, C.byref(done),
                                        it.ctypes.data, rr.ctypes.data, why.ctypes.data, 0, None, 0, None, None, None, 0)
    return rc, done.value, it, why


def test_refusals_leave_x_and_the_operator_unchanged(small):
    from otmb_amd import capi

    D, N, dage, Dk, X7, S7, F7 = small
    X0 = np.asfortranarray(X7[:, :2])
    S = np.asfortranarray(S7[:, :2])
    before = D.mul(X0)
    a, b, w = [0, 1, 2, 2], [1, 2, 0, 0], [0.5, 0.25, 0.0, 1.0]
    nsrc_text = "nsrc must be 0 or 1 (a source per slot is not built with interpolation)"
    bad = [(dict(a=None), "slot_a, slot_b or weight is null"), (dict(b=None), "slot_a, slot_b or weight is null"), (dict(w=None), "slot_a, slot_b or weight is null"),
           (dict(a=[0, 1, 4, 2]), "step 2: slot 4 is outside 0..3 (otmb_op_set_slots)"), (dict(b=[-1, 2, 0, 0]), "step 0: slot -1 is outside 0..3 (otmb_op_set_slots)"),
           (dict(w=[0.5, np.nan, 0.0, 1.0]), "step 1: the weight nan is not finite or outside [0, 1]"),
           (dict(w=[0.5, 0.25, 0.0, np.inf]), "step 3: the weight inf is not finite or outside [0, 1]"),
           (dict(w=[-0.25, 0.25, 0.0, 1.0]), "step 0: the weight -0.25 is not finite or outside [0, 1]"),
           (dict(w=[0.5, 0.25, 1.5, 1.0]), "step 2: the weight 1.5 is not finite or outside [0, 1]"),
           (dict(S=[S, S]), nsrc_text), (dict(S=[S] * 4), nsrc_text), (dict(nsrc=-1), nsrc_text),  # (four blocks: one per slot, the scheduled call's)
           (dict(S=None, nsrc=1), "S is null with nsrc > 0"), (dict(S=[None]), "a source block is null"),
           (dict(scale=np.ones((4, 2))), "scale needs a source (nsrc > 0)")]
    for kw, text in bad:
        X = X0.copy(order="F")
        args = dict(dict(a=a, b=b, w=w), **kw)
        rc, done, it, why = _interp_c(D, X, N, 2, args.pop("a"), args.pop("b"), args.pop("w"), nsteps=4, **args)
        msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
        assert rc == 11, (kw.keys(), rc, msg)
        assert np.array_equal(X, X0) and (it == -7).all() and (why == -7).all() and D.slots == (NSLOTS + 1, 0), kw.keys()
        assert msg == f"{capi.lib().otmb_status_string(11).decode()}: otmb_op_step_interp: {text}", msg
    # ... after the checks of the call they extend: with two bad arguments the older complaint comes first
    X = X0.copy(order="F")
    assert _interp_c(D, X, N, 2, a, b, [2.0, 0.0, 0.0, 0.0], dt=0.0)[0] == 11
    assert capi.lib().otmb_last_error(D.ctx.handle).decode().endswith("dt must be > 0 and finite")
    DK.same_bits(D.mul(X0), before, "the operator after the refusals")
    # and a call that is in order still runs, through the same handle
    X = X0.copy(order="F")
    rc, done, it, why = _interp_c(D, X, N, 2, a, b, w, S=[S])
    want, _ = D.step_interp(X0, dt=SR.MONTH, slot_a=a, slot_b=b, weight=w, source=S)
    assert rc == 0 and done == 4 and (why == 0).all()
    DK.same_bits(X, want, "the C call after the refusals")
    # no steps: nothing runs, nothing is read through the schedule's arrays
    assert _interp_c(D, X, N, 2, None, None, None, nsteps=0)[:2] == (0, 0)


def test_a_singular_blended_preconditioner_names_step_slots_and_weight():
    """diag(1, 1) in slot 0 and diag(-3, -3) in slot 1, σ = 1 (δt = 1, θ = 1): each slot's Jacobi diagonal is regular (2 and -2), their blend
    at w = 0.5 is -1, and σ + (-1) = 0 exactly.  Steps: plain on 0, plain on 1 (w = 1.0), blended -- the call ends there with
    OTMB_ERR_SINGULAR_PRECONDITIONER, steps_done = 2 and X the state after step 1."""
    import otmb_amd.api as api
    from otmb_amd import capi

    p, i = np.array([1, 2, 3]), np.array([1, 2])
    with api.DeviceOperator(_csc(2, p, i, np.array([1.0, 1.0]))) as Z:
        Z.set_slots(2)
        Z.set_values(np.array([-3.0, -3.0]), slot=1)
        X0 = np.asfortranarray(np.array([[1.0], [2.0]]))
        a, b, w = [0, 0, 0, 1], [0, 1, 1, 1], [0.0, 1.0, 0.5, 0.0]
        X = X0.copy(order="F")
        rc, done, it, why = _interp_c(Z, X, 2, 1, a, b, w, dt=1.0)
        msg = capi.lib().otmb_last_error(Z.ctx.handle).decode()
        assert rc == 18 and done == 2 and (why[:2] == 0).all() and (it[2:] == -7).all(), (rc, done, msg)
        assert msg.endswith("(step 2, slots 0 and 1, weight 0.5)"), msg
        want, info = Z.step(X0, dt=1.0, nsteps=2, first_slot=0)
        assert info.steps_done == 2
        DK.same_bits(X, want, "the state after step 1")
        with pytest.raises(capi.OtmbError) as e:
            Z.step_interp(X0, dt=1.0, slot_a=a, slot_b=b, weight=w)
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "step 2, slots 0 and 1, weight 0.5" in str(e.value), str(e.value)
        # the blend at another weight is regular: the same handle steps on
        Xn, info = Z.step_interp(X0, dt=1.0, slot_a=a, slot_b=b, weight=[0.0, 1.0, 0.25, 0.0])
        assert info.steps_done == 4 and Z.slots == (2, 0)


def test_the_device_route_with_padded_misaligned_tensors():
    """device.Operator.step_interp at n = 1025 (five workgroups of the row kernels, the last of one row): X's start, the source and the
    per-column d are separate tensors with a padded leading dimension and a base 8 bytes off a 16-byte boundary; the result has the bits of
    the call on compact tensors (θ = 0.5 with Aᵀ, θ = 1 with A), and at θ = 1 those of the host route."""
    import torch

    from otmb_amd import device

    n, k = 1025, 3
    p, i, v = R.dominant(n)
    dev = torch.device("cuda", 0)
    ctx = device.DeviceAssembler(0).ctx
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    X0, S, F = _start(n, k, 81), _sources(n, k, 82, size=1.0), _scale(3, k)
    Dk = np.asfortranarray(np.random.default_rng(83).uniform(0.0, 1.0, (n, k)))
    sched = dict(slot_a=[2, 0, 0], slot_b=[0, 0, 1], weight=[0.5, 0.5, 0.25])  # blended (the wrap pair), plain, blended

    def padded(a, pad=5):
        ld = n + pad
        buf = torch.full((1 + ld * k,), float("nan"), dtype=torch.float64, device=dev)
        view = buf[1:].as_strided((n, k), (1, ld))
        view.copy_(t(a.T, np.float64).t())
        assert view.data_ptr() % 16 == 8
        return view

    nxt = LR.random_lines(n, 3)
    with _operator(n, p, i, v, nxt=nxt) as D, device.Operator(ctx, n, n, t(p, np.int64), t(i, np.int64), t(v, np.float64)) as O:
        O.set_slots(NSLOTS)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            O.set_values_dev(t(vals, np.float64), slot=s)
        O.set_lines(t(nxt, np.int64))
        compact = [t(a.T, np.float64).t() for a in (X0, S, Dk)]
        pads = [padded(a) for a in (X0, S, Dk)]
        for theta, adjoint in ((0.5, True), (1.0, False)):
            kw = dict(dt=2.0, theta=theta, source_scale=F, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines", **sched)
            Xc, ic = O.step_interp(compact[0], source=compact[1], d=compact[2], **kw)
            Xp, ip = O.step_interp(pads[0], source=pads[1], d=pads[2], **kw)
            assert ic.steps_done == ip.steps_done == 3
            DK.same_bits(Xp.cpu().numpy(), Xc.cpu().numpy(), ("padded and misaligned", theta, adjoint))
            assert np.array_equal(ip.iterations, ic.iterations)
            if theta == 1.0:
                Xh, ih = D.step_interp(X0, source=S, d=Dk, **kw)
                DK.same_bits(Xc.cpu().numpy(), Xh, ("device route against the host route", theta, adjoint))
                assert ih.steps_done == 3 and np.array_equal(ic.iterations, ih.iterations)
        assert O.slots == (NSLOTS, 0)
