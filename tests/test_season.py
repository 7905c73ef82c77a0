"""GPU: otmb_op_step_season (csrc/otmb_step.hip, csrc/otmb_season.hip): θ-steps whose matrix, d and source follow the slots and are blended
with the step's own weights.  The contract of include/otmb.h in PUBLIC calls on the same operator, which has one slot more than the cycle as
the chain's scratch: step t has the bits of combine_slots() into the scratch slot (on a blended step) followed by the one-step step() with
d_t and s_t·scale[t], both blended in numpy by the three stated statements (tests/season_ref.py: field) -- states, steps_done, iterations,
relres, reasons.  With at most one block of each the call has the bits of step_interp; with plain_schedule, one d and a source per slot those
of step_sched.  A column of seven is the column alone; the record is that of the chain's states; refusals leave everything as it was; a
preconditioner made singular by d alone names its step, both slots and the weight.

The fold kernel at its edges: solve_ref.dominant(n) operators make n free, so n lies below one workgroup's span of rows, one above a span,
and odd beyond two spans; k = 3 with a d per column, so with an odd n every second column starts 8 bytes off a 16-byte boundary; and the
blocks are separate device tensors, padded by 5, whose bases lie alternately 0 and 8 bytes off a 16-byte boundary from block to block --
so in one launch some columns take the 16-byte path and others the 8-byte one, and the bits are those of the compact call."""
import ctypes as C

import numpy as np
import pytest

import dk_cases as DK
import observe_ref as OR
import season_ref as SN
import interp_ref as IR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_interp import HAND, NSLOTS, NSTEPS, SPARE, _operator, _scale, _sources
from test_step import _csc, _start

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
SE_SPAN = 2048  # csrc/otmb_season.hip: rows of one column per workgroup of the fold kernel
DSCALE, SSCALE = (1.0, 0.5, 0.125), (1.0, 0.5, 1.5)


def _blocks(a, scales, count):
    """None (count 0), the one block (1), or a block per slot: a·scales[s], column-major, and for the chain's scratch slot, which no schedule
    names, a block of NaN: it is never read."""
    if count == 0:
        return None
    blocks = [np.asfortranarray(a * f) if a.ndim == 2 else a * f for f in scales[:count]]
    return blocks if count == 1 else blocks + [np.full_like(blocks[0], np.nan)]


def _chain(D, X0, sched, *, d, sources, scale, **kw):
    """The contract in public calls.  -> (X, steps_done, rows, the states after every completed step)"""
    X, done, rows, states = np.array(X0, order="F"), 0, [], []
    for t, (a, b, w) in enumerate(zip(*sched)):
        what, slot = IR.kind(int(a), int(b), float(w))
        if what == "blend":
            D.combine_slots(IR.combine_weights(NSLOTS + 1, int(a), int(b), float(w)), SPARE)
            slot = SPARE
        X, info = D.step(X, nsteps=1, first_slot=slot, source=SN.source_of(sources, scale, t, a, b, w), d=SN.field(d, a, b, w), **kw)
        rows.append((info.iterations[0], info.relres[0], info.reason[0]))
        if info.steps_done != 1:
            break
        done = t + 1
        states.append(X)
    return X, done, rows, states


def _same_as_the_chain(D, X0, sched, what, *, d=None, sources=None, scale=None, may_stop=False, **kw):
    """may_stop: a step whose solve does not converge may end the call -- the chain then ends at the same step with the same report and the
    same last iterates; otherwise every step must be completed."""
    Xs, info = D.step_season(X0, slot_a=sched[0], slot_b=sched[1], weight=sched[2], d=d, source=sources, source_scale=scale, **kw)
    Xc, done, rows, states = _chain(D, X0, sched, d=d, sources=sources, scale=scale, **kw)
    nsteps = len(sched[2])
    assert info.steps_done == done and len(info.reason) == len(rows) and done >= (1 if may_stop else nsteps), (what, info)
    if done == nsteps:
        assert info.status == 0 and all(r == "converged" for row in info.reason for r in row), (what, info.reason)
    DK.same_bits(Xs, Xc, (what, "state"))
    for t, (it, rr, why) in enumerate(rows):
        assert np.array_equal(info.iterations[t], it) and info.reason[t] == why, (what, t)
        DK.same_bits(info.relres[t], rr, (what, t, "relres"))
    return Xs, info, states


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117, odd: below one span of the fold kernel, every second column of an n x k block 8 bytes off), 3 + 1 slots and the
    water columns; the age d and the seven-column D; a start, a source of seven columns and a history of 8 x 7."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    assert N % 2 == 1 and N < SE_SPAN
    D = _operator(N, *T, nxt=nxt)
    yield D, N, R.shift("age", N, nsurf)[0], DK.columns(N, nsurf, zero=True), _start(N, 7, 12), _sources(N, 7, 11), _scale(NSTEPS, 7)
    D.close()


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_season_step_has_the_bits_of_the_chain_of_public_calls(small, theta, adjoint, precond):
    """N = 117, the hand-written eight steps (HAND: plain, blend, w = 0, w = 1, the wrap pair (2, 0), w = 1/3): k = 1, 3, 7 (register blocks
    1; 2 + 1; 4 + 2 + 1) x nd in {0, 1, nslots} x nsrc in {0, 1, nslots}; with a source, with and without a history in turn; with d, shared
    (ldd = 0) and per column in turn (a 1-D state has no per-column d).  With the lines all 27 combinations run; Jacobi's solves take
    hundreds of iterations a step here, so it runs nine of them, chosen so that every nd and every nsrc meets every k.  Without d the
    θ = 0.5 Jacobi systems of this grid can break BiCGStab down: such a call may end early, at the chain's step with the chain's bits.
    With nd <= 1 and nsrc <= 1 the call also has the bits of step_interp; with plain_schedule, one d and a source per slot those of
    step_sched."""
    from otmb_amd import api

    D, N, dage, Dk, X7, S7, F7 = small
    kw = dict(dt=SR.MONTH, theta=theta, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
    turn = 0
    for ki, k in enumerate((1, 3, 7)):
        X0 = X7[:, 0] if k == 1 else X7[:, :k]
        S = S7[:, 0] if k == 1 else S7[:, :k]
        for di, nd in enumerate((0, 1, NSLOTS)):
            for si, nsrc in enumerate((0, 1, NSLOTS)):
                turn += 1
                if precond == "jacobi" and (di + si) % 3 != ki:
                    continue
                percol = k > 1 and turn % 2 == 0
                d = _blocks(np.asfortranarray(Dk[:, :k]) if percol else dage, DSCALE, nd)
                sources = _blocks(S, SSCALE, nsrc)
                scale = None if nsrc == 0 or turn % 3 == 0 else F7[:, 0] if k == 1 else np.ascontiguousarray(F7[:, :k])
                what = (theta, adjoint, precond, k, nd, nsrc, percol, scale is not None)
                Xs, info, _ = _same_as_the_chain(D, X0, HAND, what, d=d, sources=sources, scale=scale,
                                                 may_stop=nd == 0 and precond == "jacobi" and theta == 0.5, **kw)
                if nd <= 1 and nsrc <= 1:
                    Xi, ii = D.step_interp(X0, slot_a=HAND[0], slot_b=HAND[1], weight=HAND[2], d=None if d is None else d[0],
                                           source=None if sources is None else sources[0], source_scale=scale, **kw)
                    DK.same_bits(Xs, Xi, (what, "step_interp"))
                    assert np.array_equal(info.iterations, ii.iterations) and ii.steps_done == info.steps_done
                    DK.same_bits(info.relres, ii.relres, (what, "step_interp: relres"))
    # the explicit plain schedule is the scheduled step's: 5 steps from slot 0 with two sub-steps (slots 0, 0, 1, 1, 2), one d, a source per
    # slot, a history
    X0, sources, scale = X7[:, :3], _blocks(S7[:, :3], SSCALE, NSLOTS), np.ascontiguousarray(F7[:5, :3])
    a, b, w = api.plain_schedule(NSLOTS + 1, 5, substeps=2)
    assert a.tolist() == [0, 0, 1, 1, 2]
    Xs, info = D.step_season(X0, slot_a=a, slot_b=b, weight=w, d=dage, source=sources, source_scale=scale, **kw)
    Xq, iq = D.step_sched(X0, nsteps=5, substeps=2, d=dage, source=sources, source_scale=scale, **kw)
    DK.same_bits(Xs, Xq, "plain_schedule against step_sched")
    assert np.array_equal(info.iterations, iq.iterations) and info.steps_done == iq.steps_done == 5
    DK.same_bits(info.relres, iq.relres, "plain_schedule against step_sched: relres")
    assert D.slots == (NSLOTS + 1, 0)  # the selection is the caller's


@pytest.mark.parametrize("n", [1025, SE_SPAN + 1, 2 * SE_SPAN + 3])
def test_the_fold_kernel_at_its_edges(n):
    """device.Operator.step_season with a d per column and per slot and a source per slot, k = 3: n = 1025 (below one span of the fold
    kernel), n = SE_SPAN + 1 (a second workgroup of one row per column) and n = 2·SE_SPAN + 3 (odd, beyond two spans).  The state, the three D
    blocks and the three S blocks are separate tensors with a leading dimension padded by 5 whose bases lie alternately 0 and 8 bytes off a
    16-byte boundary from block to block; the result has the bits of the call on compact tensors, and at θ = 1 those of the host route."""
    import torch

    from otmb_amd import device

    k = 3
    dev = torch.device("cuda", 0)
    ctx = device.DeviceAssembler(0).ctx
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    sched = dict(slot_a=[2, 0, 0, 1], slot_b=[0, 0, 1, 2], weight=[0.5, 0.5, 0.25, 1.0 / 3.0])  # blended (the wrap pair), plain, blended, blended

    def padded(a, off, pad=5):
        n = a.shape[0]
        ld = n + pad
        buf = torch.full((2 + ld * k,), float("nan"), dtype=torch.float64, device=dev)
        first = (off - buf.data_ptr() // 8) % 2  # the view's base: `off` doubles past a 16-byte boundary
        view = buf[first:].as_strided((n, k), (1, ld))
        view.copy_(t(a.T, np.float64).t())
        assert view.data_ptr() % 16 == 8 * off
        return view

    assert (n < SE_SPAN) if n == 1025 else (n == SE_SPAN + 1) if n < 2 * SE_SPAN else (n % 2 == 1 and n > 2 * SE_SPAN)
    p, i, v = R.dominant(n)
    X0, S, F = _start(n, k, 81), _sources(n, k, 82, size=1.0), _scale(4, k)
    Dk = np.asfortranarray(np.random.default_rng(83).uniform(0.0, 1.0, (n, k)))
    Ds, Ss = [np.asfortranarray(Dk * f) for f in DSCALE], [np.asfortranarray(S * f) for f in SSCALE]
    nxt = LR.random_lines(n, 3)
    with device.Operator(ctx, n, n, t(p, np.int64), t(i, np.int64), t(v, np.float64)) as O:
        O.set_slots(NSLOTS)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            O.set_values_dev(t(vals, np.float64), slot=s)
        O.set_lines(t(nxt, np.int64))
        compact = lambda a: t(a.T, np.float64).t()
        Xc0, Dc, Sc = compact(X0), [compact(a) for a in Ds], [compact(a) for a in Ss]
        Xp0, Dp, Sp = padded(X0, 1), [padded(a, j % 2) for j, a in enumerate(Ds)], [padded(a, (j + 1) % 2) for j, a in enumerate(Ss)]
        assert [x.data_ptr() % 16 for x in Dp] == [0, 8, 0] and [x.data_ptr() % 16 for x in Sp] == [8, 0, 8]
        for theta, adjoint in ((0.5, True), (1.0, False)):
            kw = dict(dt=2.0, theta=theta, source_scale=F, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines", **sched)
            Xc, ic = O.step_season(Xc0, d=Dc, source=Sc, **kw)
            Xp, ip = O.step_season(Xp0, d=Dp, source=Sp, **kw)
            assert ic.steps_done == ip.steps_done == 4
            DK.same_bits(Xp.cpu().numpy(), Xc.cpu().numpy(), ("padded and misaligned", n, theta, adjoint))
            assert np.array_equal(ip.iterations, ic.iterations)
            if theta == 1.0:
                with api_operator(n, p, i, v, nxt) as D:
                    Xh, ih = D.step_season(X0, d=Ds, source=Ss, **kw)
                DK.same_bits(Xc.cpu().numpy(), Xh, ("device route against the host route", n))
                assert ih.steps_done == 4 and np.array_equal(ic.iterations, ih.iterations)
        assert O.slots == (NSLOTS, 0)


def api_operator(n, p, i, v, nxt):
    """A DeviceOperator with exactly the cycle's three slots (no scratch slot) and the lines."""
    import otmb_amd.api as api

    D = api.DeviceOperator(_csc(n, p, i, v))
    D.set_slots(NSLOTS)
    for s, vals in enumerate(SR.slot_values(v, seed=1)):
        D.set_values(vals, slot=s)
    D.set_lines(nxt)
    return D


def test_a_fold_beyond_one_span_has_the_bits_of_the_chain():
    """n = 2·SE_SPAN + 3, k = 3, the host route against the chain of public calls with the numpy blend: what the kernel computes beyond its
    first workgroup, in columns on either access width, is the three stated statements."""
    n, k = 2 * SE_SPAN + 3, 3
    p, i, v = R.dominant(n)
    X0, S, F = _start(n, k, 81), _sources(n, k, 82, size=1.0), _scale(3, k)
    Dk = np.asfortranarray(np.random.default_rng(83).uniform(0.0, 1.0, (n, k)))
    sched = (np.array([2, 0, 0]), np.array([0, 0, 1]), np.array([0.5, 0.5, 1.0 / 3.0]))
    with _operator(n, p, i, v) as D:
        _same_as_the_chain(D, X0, sched, "beyond two spans", d=_blocks(Dk, DSCALE, NSLOTS), sources=_blocks(S, SSCALE, NSLOTS), scale=F, dt=2.0, theta=0.5,
                           rtol=RTOL, maxiter=MAXITER, adjoint=True, precond="jacobi")
        assert D.slots == (NSLOTS + 1, 0)


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_a_column_alone_and_the_record(small, theta, precond):
    """k = 7 with a D per column and per slot, a source per slot and a history: columns 0, 3 and 6 (the first of the block of four, its last,
    the block of one) have the bits of the column stepped alone with its own column of every block.  With observers and time weights, X and
    the report are the plain call's, the observations are observe() of the chain's states and the mean is observe_ref.mean_ref of them."""
    D, N, dage, Dk, X7, S7, F7 = small
    sched = dict(slot_a=HAND[0], slot_b=HAND[1], weight=HAND[2])
    kw = dict(dt=SR.MONTH, theta=theta, rtol=RTOL, maxiter=MAXITER, precond=precond, adjoint=theta == 0.5)
    Ds, Ss = _blocks(np.asfortranarray(Dk), DSCALE, NSLOTS), _blocks(S7, SSCALE, NSLOTS)
    Xs, info = D.step_season(X7, source=Ss, source_scale=F7, d=Ds, **sched, **kw)
    assert info.steps_done == NSTEPS
    for c in (0, 3, 6):
        xc, ic = D.step_season(X7[:, c], source=[np.ascontiguousarray(S[:, c]) for S in Ss], source_scale=np.ascontiguousarray(F7[:, c]),
                               d=[np.ascontiguousarray(x[:, c]) for x in Ds], **sched, **kw)
        DK.same_bits(xc, Xs[:, c], ("column alone", c))
        assert np.array_equal(ic.iterations[:, 0], info.iterations[:, c]) and ic.steps_done == NSTEPS
        DK.same_bits(ic.relres[:, 0], info.relres[:, c], ("column alone: relres", c))
    assert not np.array_equal(Xs[:, 0], Xs[:, 3])
    rng = np.random.default_rng(71)
    W, tw = np.asfortranarray(rng.uniform(0.0, 1.0, (N, 3))), rng.uniform(0.0, 1.0, NSTEPS)
    X0, F = X7[:, :3], np.ascontiguousarray(F7[:, :3])
    d3, S3 = _blocks(dage, DSCALE, NSLOTS), _blocks(S7[:, :3], SSCALE, NSLOTS)
    Xp, ip = D.step_season(X0, source=S3, source_scale=F, d=d3, **sched, **kw)
    Xr, ir = D.step_season(X0, source=S3, source_scale=F, d=d3, observe=W, time_weights=tw, **sched, **kw)
    _, done, _, states = _chain(D, X0, HAND, d=d3, sources=S3, scale=F, **kw)
    assert ip.observations is None and ip.mean is None and done == NSTEPS
    DK.same_bits(Xr, Xp, "X with a record")
    assert np.array_equal(ir.iterations, ip.iterations) and ir.steps_done == NSTEPS
    DK.same_bits(ir.relres, ip.relres, "relres with a record")
    assert ir.observations.shape == (NSTEPS, 3, 3)
    for t, Xt in enumerate(states):
        DK.same_bits(ir.observations[t], D.observe(W, Xt).T, ("observations", t))
    DK.same_bits(ir.mean, OR.mean_ref(states, tw), "the mean")
    assert D.slots == (NSLOTS + 1, 0)


def _season_c(D, X, ldx, k, a, b, w, *, Dl=(), nd=None, ldd=0, S=(), nsrc=None, lds=None, scale=None, dt=SR.MONTH, theta=1.0, precond=0, nsteps=None):
    """otmb_op_step_season through the C ABI; a, b, w: arrays or None (a null array); Dl, S: sequences of arrays (an entry None: a null block),
    or None (a null array).  -> (status, steps_done, iters, reason) with the report preset to sentinels."""
    from otmb_amd import capi

    nsteps = max(len(x) for x in (a, b, w) if x is not None) if nsteps is None else nsteps
    it, rr, why = np.full((max(nsteps, 1), k), -7, np.int64), np.full((max(nsteps, 1), k), 7.25), np.full((max(nsteps, 1), k), -7, np.int32)
    done = C.c_int64(-7)
    a, b = (None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (a, b))
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    arr = lambda L: None if L is None else (C.c_void_p * max(len(L), 1))(*[None if s is None else s.ctypes.data for s in L])
    ptr = lambda x: None if x is None else x.ctypes.data
    rc = capi.lib().otmb_op_step_season(D.handle, 0, k, len(Dl) if nd is None else nd, arr(Dl), ldd, float(dt), float(theta), nsteps, ptr(a), ptr(b), ptr(w),
                                        len(S) if nsrc is None else nsrc, arr(S), (X.shape[0] if lds is None else lds), ptr(scale), X.ctypes.data, ldx,
                                        RTOL, MAXITER, precond, C.byref(done), it.ctypes.data, rr.ctypes.data, why.ctypes.data, 0, None, 0, None, None, None, 0)
    return rc, done.value, it, why


def test_refusals_leave_x_and_the_operator_unchanged(small):
    from otmb_amd import capi

    D, N, dage, Dk, X7, S7, F7 = small
    X0, S, D2 = np.asfortranarray(X7[:, :2]), np.asfortranarray(S7[:, :2]), np.asfortranarray(Dk[:, :2])
    before = D.mul(X0)
    a, b, w = [0, 1, 2, 2], [1, 2, 0, 0], [0.5, 0.25, 0.0, 1.0]
    nd_text, ldd_text = "nd must be 0, 1 or the number of slots", "ldd must be 0 (the n values of a block serve every column) or >= n"
    bad = [(dict(Dl=[dage] * 2), nd_text), (dict(Dl=[dage] * 3), nd_text), (dict(nd=-1), nd_text), (dict(Dl=[dage] * 5), nd_text),
           (dict(Dl=None, nd=1), "D is null with nd > 0"), (dict(Dl=[None]), "a d block is null"), (dict(Dl=[dage, dage, None, dage]), "a d block is null"),
           (dict(Dl=[D2], ldd=N - 1), ldd_text), (dict(Dl=[D2] * 4, ldd=1), ldd_text), (dict(Dl=[D2], ldd=-N), ldd_text),
           # what the interpolated call refuses, under this call's name -- except a source per slot, which is in order
           (dict(S=[S, S]), "nsrc must be 0, 1 or the number of slots"), (dict(nsrc=-1), "nsrc must be 0, 1 or the number of slots"),
           (dict(S=None, nsrc=1), "S is null with nsrc > 0"), (dict(S=[S, None, S, S]), "a source block is null"), (dict(S=[S], lds=N - 1), None),
           (dict(scale=np.ones((4, 2))), "scale needs a source (nsrc > 0)"), (dict(a=None), "slot_a, slot_b or weight is null"),
           (dict(a=[0, 1, 4, 2]), "step 2: slot 4 is outside 0..3 (otmb_op_set_slots)"),
           (dict(w=[0.5, 0.25, 1.5, 1.0]), "step 2: the weight 1.5 is not finite or outside [0, 1]"),
           # the schedule's complaint comes before the d blocks'
           (dict(w=[0.5, np.nan, 0.0, 1.0], Dl=[dage] * 2), "step 1: the weight nan is not finite or outside [0, 1]")]
    for kw, text in bad:
        X = X0.copy(order="F")
        args = dict(dict(a=a, b=b, w=w), **kw)
        rc, done, it, why = _season_c(D, X, N, 2, args.pop("a"), args.pop("b"), args.pop("w"), nsteps=4, **args)
        msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
        assert rc == 11, (kw.keys(), rc, msg)
        assert np.array_equal(X, X0) and (it == -7).all() and (why == -7).all() and D.slots == (NSLOTS + 1, 0), kw.keys()
        if text is not None:
            assert msg == f"{capi.lib().otmb_status_string(11).decode()}: otmb_op_step_season: {text}", msg
    # ... after the checks of the call they extend: with two bad arguments the older complaint comes first
    X = X0.copy(order="F")
    assert _season_c(D, X, N, 2, a, b, w, Dl=[dage] * 2, dt=0.0)[0] == 11
    assert capi.lib().otmb_last_error(D.ctx.handle).decode().endswith("dt must be > 0 and finite")
    DK.same_bits(D.mul(X0), before, "the operator after the refusals")
    # and a call that is in order still runs, through the same handle: a block per slot of each, the scratch slot's never read
    Ds, Ss = [D2 * f for f in DSCALE] + [np.full_like(D2, np.nan)], [S * f for f in SSCALE] + [np.full_like(S, np.nan)]
    Ds, Ss = [np.asfortranarray(x) for x in Ds], [np.asfortranarray(x) for x in Ss]
    X = X0.copy(order="F")
    rc, done, it, why = _season_c(D, X, N, 2, a, b, w, Dl=Ds, ldd=N, S=Ss)
    want, _ = D.step_season(X0, dt=SR.MONTH, slot_a=a, slot_b=b, weight=w, d=Ds, source=Ss)
    assert rc == 0 and done == 4 and (why == 0).all()
    DK.same_bits(X, want, "the C call after the refusals")
    assert _season_c(D, X, N, 2, None, None, None, nsteps=0)[:2] == (0, 0)  # no steps: nothing runs, nothing is read through the arrays


def test_a_blended_preconditioner_made_singular_by_d_alone_names_step_slots_and_weight():
    """diag(1, 1) in both slots, D_0 = 0 and D_1 = -4, σ = 1 (δt = 1, θ = 1): plain on slot 0 the Jacobi diagonal is 2, plain on slot 1 it is
    -2, and the blend at w = 0.5 has d = -2 and σ + d + 1 = 0 exactly.  Steps: plain on 0, plain on 1 (w = 1.0), blended -- the call ends
    there with OTMB_ERR_SINGULAR_PRECONDITIONER, steps_done = 2 and X the state after step 1; at w = 0.25 the same handle steps on."""
    import otmb_amd.api as api
    from otmb_amd import capi

    p, i = np.array([1, 2, 3]), np.array([1, 2])
    with api.DeviceOperator(_csc(2, p, i, np.array([1.0, 1.0]))) as Z:
        Z.set_slots(2)
        Z.set_values(np.array([1.0, 1.0]), slot=1)
        Dl = [np.array([0.0, 0.0]), np.array([-4.0, -4.0])]
        X0 = np.asfortranarray(np.array([[1.0], [2.0]]))
        a, b, w = [0, 0, 0, 1], [0, 1, 1, 1], [0.0, 1.0, 0.5, 0.0]
        X = X0.copy(order="F")
        rc, done, it, why = _season_c(Z, X, 2, 1, a, b, w, Dl=Dl, dt=1.0)
        msg = capi.lib().otmb_last_error(Z.ctx.handle).decode()
        assert rc == 18 and done == 2 and (why[:2] == 0).all() and (it[2:] == -7).all(), (rc, done, msg)
        assert msg.endswith("(step 2, slots 0 and 1, weight 0.5)"), msg
        x1, i1 = Z.step(X0, dt=1.0, nsteps=1, first_slot=0, d=Dl[0])
        want, i2 = Z.step(x1, dt=1.0, nsteps=1, first_slot=1, d=Dl[1])
        assert i1.steps_done == i2.steps_done == 1
        DK.same_bits(X, want, "the state after step 1")
        with pytest.raises(capi.OtmbError) as e:
            Z.step_season(X0, dt=1.0, slot_a=a, slot_b=b, weight=w, d=Dl)
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "step 2, slots 0 and 1, weight 0.5" in str(e.value), str(e.value)
        # the matrices alone are regular on every step: without the d blocks the same schedule runs through
        _, info = Z.step_interp(X0, dt=1.0, slot_a=a, slot_b=b, weight=w)
        assert info.steps_done == 4
        Xn, info = Z.step_season(X0, dt=1.0, slot_a=a, slot_b=b, weight=[0.0, 1.0, 0.25, 0.0], d=Dl)
        assert info.steps_done == 4 and Z.slots == (2, 0)
