"""The periodic state of the stepped cycle on the device (csrc/otmb_periodic.hip; otmb_op_periodic[_dev]): restarted GMRES on the cycle map.
Every answer is judged by step() itself -- one more cycle from the returned state, ‖F(x) - x‖₂ <= ptol·‖g‖₂ -- and against the dense fixed
point (I - Φ)⁻¹·g of tests/periodic_ref.py; a column of k has the bits of the column alone; refusals, maxcycles, a NaN column, padded device
arrays and the assembler's route.  Every fixture here has n <= 429, one workgroup of the file's kernels (PD_ROWS = 2048 rows) and one row
pair a lane: tests/test_periodic_rows.py runs the sizes above that, bit for bit against the restatement in the device's order."""
import ctypes as C

import numpy as np
import pytest

import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _csc, _operator, _same_bits, _start

pytestmark = pytest.mark.gpu

RTOL, PTOL, MAXITER = 1e-12, 1e-8, 5000
FIRST = 2
SENTINEL = 7.25


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117) with the tests' three slots and the water columns, the age d, the source of seven columns (ones, then random)."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    D = _operator(N, *T, nxt=nxt)
    yield D, N, T, R.shift("age", N, nsurf)[0], _start(N, 7, 101)
    D.close()


_REF = {}


def _reference(N, T, d, S, theta, adjoint, ncycle, first_slot=FIRST):
    """Computed once per (θ, adjoint, ncycle): the dense cycle, x*, ‖g‖, ‖(I - Φ)⁻¹‖₂ and max_t ‖b_t‖ along the cycle from x*."""
    key = (N, theta, adjoint, ncycle, first_slot, S.shape[1])
    if key not in _REF:
        DC = PR.DenseCycle(N, T[0], T[1], SR.slot_values(T[2], seed=1), dt=SR.MONTH, theta=theta, ncycle=ncycle, first_slot=first_slot, d=d,
                           adjoint=adjoint)
        xs, gnorm, ninv = DC.fixed_point(S)
        _REF[key] = (DC, xs, gnorm, ninv, DC.rhs_norms(xs, S))
    return _REF[key]


def _judge(D, X, info, S, d, ref, what, *, theta, adjoint, precond, ncycle, first_slot=FIRST):
    """One more cycle of step() from X and from zero: ‖F(x) - x‖₂ <= ptol·‖g‖₂·(1 + 1e-6); and ‖x - x*‖₂ <= ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + the
    inner-solve allowance ncycle·rtol·max_t‖b_t‖₂/σ)."""
    DC, xs, gnorm, ninv, bmax = ref
    kw = dict(dt=SR.MONTH, theta=theta, nsteps=ncycle, first_slot=first_slot, d=d, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
    X = X.reshape(len(X), -1)
    k = X.shape[1]
    FX, si = D.step(X, source=S[:, :k], **kw)
    G, sg = D.step(np.zeros_like(X), source=S[:, :k], **kw)
    assert si.status == 0 and sg.status == 0
    for c in range(k):
        defect, g = np.linalg.norm(FX[:, c] - X[:, c]), np.linalg.norm(G[:, c])
        err = np.linalg.norm(X[:, c] - xs[:, c])
        bound = ninv * (PTOL * g + ncycle * RTOL * bmax[c] / DC.sigma)
        print(what, "column", c, "cycles", int(info.cycles[c]), "defect", defect / g, "reported", info.defect[c], "error", err, "bound", bound)
        assert defect <= PTOL * g * (1 + 1e-6), (what, c, defect / g)
        assert err <= bound, (what, c, err, bound)
        assert abs(g - gnorm[c]) <= 1e-6 * gnorm[c]  # (the dense cycle is the device's cycle)


@pytest.mark.parametrize("restart", [5, 40])
@pytest.mark.parametrize("ncycle", [3, 7])
@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("k", [1, 3, 7])
def test_the_periodic_state_on_the_small_grid(small, k, theta, adjoint, precond, ncycle, restart):
    """odd_nx_fold: k = 1, 3, 7 x θ = 1, 0.5 x A, Aᵀ x both preconditioners x cycles of 3 and 7 steps (7 is no multiple of the 3 slots) from
    slot 2 x GMRES(5) (several restarts) and GMRES(40) (none at θ = 1); the age d, δt = a month, rtol = 1e-12, ptol = 1e-8."""
    D, N, T, d, S7 = small
    S = S7[:, :k]
    X, info = D.periodic(S, dt=SR.MONTH, ncycle=ncycle, theta=theta, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond,
                         ptol=PTOL, restart=restart, maxcycles=1000)
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
    assert D.slots == (3, 0)
    if restart == 40 and theta == 1.0:
        assert (info.cycles <= 42).all()  # g, at most 40 iterations, one verification
    _judge(D, X, info, S7, d, _reference(N, T, d, S7, theta, adjoint, ncycle), (k, theta, adjoint, precond, ncycle, restart), theta=theta, adjoint=adjoint,
           precond=precond, ncycle=ncycle)


@pytest.mark.parametrize("theta,precond,restart", [(1.0, "lines", 5), (0.5, "jacobi", 40)])
def test_a_column_of_seven_has_the_bits_of_the_column_alone(small, theta, precond, restart):
    """Columns 0, 3 and 6 of the k = 7 call: X, cycles and defect are those of the column solved alone (the columns stop at different cycles,
    so the calls' step calls differ in width throughout); and the same call twice gives the same bits."""
    D, N, T, d, S7 = small
    kw = dict(dt=SR.MONTH, ncycle=3, theta=theta, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, precond=precond, ptol=PTOL, restart=restart)
    X, info = D.periodic(S7, **kw)
    X2, info2 = D.periodic(S7, **kw)
    assert info.converged.all()
    _same_bits(X, X2, "the same call twice")
    _same_bits(info.defect, info2.defect, "the same call twice: defect")
    assert np.array_equal(info.cycles, info2.cycles)
    for c in (0, 3, 6):
        xc, ic = D.periodic(S7[:, c], **kw)
        print("column", c, "cycles", int(ic.cycles[0]), "of", info.cycles.tolist())
        _same_bits(xc, X[:, c], ("column alone", c))
        _same_bits(ic.defect[0], info.defect[c], ("column alone: defect", c))
        assert ic.cycles[0] == info.cycles[c]


def test_the_larger_grid(oracle):
    """tiny_tripolar (N = 429), θ = 1, twelve steps a cycle, lines, GMRES(30), maxcycles = 400: it converges (the unrestarted CPU run took
    76 iterations, GMRES(20) 116)."""
    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    d = R.shift("age", N, nsurf)[0]
    S = _start(N, 2, 111)
    with _operator(N, *T, nxt=nxt) as D:
        X, info = D.periodic(S, dt=SR.MONTH, ncycle=12, theta=1.0, first_slot=0, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=30,
                             maxcycles=400)
        print("tiny_tripolar", info)
        assert info.status == 0 and (info.cycles <= 400).all()
        _judge(D, X, info, S, d, _reference(N, T, d, S, 1.0, False, 12, first_slot=0), "tiny_tripolar", theta=1.0, adjoint=False, precond="lines", ncycle=12,
               first_slot=0)


def test_from_the_fixed_point_one_cycle_and_without_a_source_none(small):
    D, N, T, d, S7 = small
    S = S7[:, :3]
    kw = dict(dt=SR.MONTH, ncycle=3, theta=0.5, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=40)
    X, info = D.periodic(S, **kw)
    assert info.converged.all()
    X1, info1 = D.periodic(S, x0=X, **kw)
    assert info1.status == 0 and info1.cycles.tolist() == [1, 1, 1] and info1.converged.all()
    _same_bits(X1, X, "the fixed point is returned as it is")
    _same_bits(info1.defect, info.defect, "and its defect is the one it was accepted on")
    # no source, through the C ABI (S = NULL): X = 0 whatever it held, zero cycles
    rc, Xz, cyc, dft, why = _periodic_c(D, np.full((N, 2), SENTINEL, order="F"), N, 2, d=d)
    assert rc == 0 and not Xz.any() and (cyc == 0).all() and (dft == 0.0).all() and (why == 0).all()
    # a zero column of a source: the same, beside a column that iterates
    Sz = np.asfortranarray(S.copy())
    Sz[:, 1] = 0.0
    Xs, infos = D.periodic(Sz, x0=X, **kw)
    assert infos.cycles[1] == 0 and infos.reason[1] == "converged" and not Xs[:, 1].any()
    _same_bits(Xs[:, [0, 2]], X[:, [0, 2]], "the neighbours of a zero column")


def _periodic_c(D, X, ldx, k, *, S=None, lds=None, d=None, dt=SR.MONTH, theta=1.0, ncycle=3, first_slot=0, use_x0=0, rtol=RTOL, maxiter=MAXITER, precond=0,
                adjoint=0, ptol=PTOL, restart=10, maxcycles=100):
    """otmb_op_periodic through the C ABI.  -> (status, X, cycles, defect, reason) with the report arrays preset to sentinels."""
    from otmb_amd import capi

    cyc, dft, why = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32)
    rc = capi.lib().otmb_op_periodic(D.handle, adjoint, k, None if d is None else d.ctypes.data, float(dt), float(theta), ncycle, first_slot,
                                     None if S is None else S.ctypes.data, 0 if lds is None else lds, None if X is None else X.ctypes.data, ldx, use_x0,
                                     float(rtol), maxiter, precond, float(ptol), restart, maxcycles, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data)
    return rc, X, cyc, dft, why


def test_refusals_leave_x_the_selection_and_the_operator_as_they_were(small):
    import otmb_amd.api as api
    from otmb_amd import capi

    D, N, T, d, S7 = small
    S = np.asfortranarray(S7[:, :2])
    X0 = _start(N, 2, 121)
    before = D.mul(X0)
    D.select(1)
    bad = [dict(ptol=0.0), dict(ptol=-1.0), dict(ptol=float("nan")), dict(restart=0), dict(restart=-2), dict(maxcycles=-1), dict(first_slot=3),
           dict(first_slot=-1), dict(ncycle=0), dict(dt=0.0), dict(theta=1.5), dict(rtol=0.0), dict(maxiter=-1), dict(precond=2), dict(lds=N - 1)]
    for kw in bad:
        X = X0.copy(order="F")
        rc, _, cyc, dft, why = _periodic_c(D, X, N, 2, **dict(dict(S=S, lds=N, use_x0=1), **kw))
        assert rc == 11, kw
        assert np.array_equal(X, X0) and (cyc == -7).all() and (dft == SENTINEL).all() and (why == -7).all() and D.slots == (3, 1), kw
    # two bad arguments at once: the complaint is the first in the checks' order
    slot_text = "first_slot is not a slot of the operator (otmb_op_set_slots)"
    for kw, first in ((dict(rtol=0.0, dt=0.0), "rtol must be > 0"), (dict(theta=0.0, first_slot=99), "theta must be in (0, 1]"),
                      (dict(ncycle=0, first_slot=99), "ncycle must be >= 1"), (dict(first_slot=99, ptol=0.0), slot_text)):
        X = X0.copy(order="F")
        assert _periodic_c(D, X, N, 2, **dict(dict(S=S, lds=N, use_x0=1), **kw))[0] == 11, kw
        assert capi.lib().otmb_last_error(D.ctx.handle).decode() == f"{capi.lib().otmb_status_string(11).decode()}: {first}", kw
        assert np.array_equal(X, X0) and D.slots == (3, 1), kw
    X = X0.copy(order="F")
    assert _periodic_c(D, X, N - 1, 2, S=S, lds=N)[0] == 11 and _periodic_c(D, X, N, 0, S=S, lds=N)[0] == 11 and _periodic_c(D, None, N, 2, S=S, lds=N)[0] == 11
    assert capi.lib().otmb_op_periodic(D.handle, 0, 2, None, 1.0, 1.0, 3, 0, S.ctypes.data, N, X.ctypes.data, N, 0, RTOL, 10, 0, PTOL, 5, 10, None, None,
                                       None) == 11
    assert np.array_equal(X, X0)
    with pytest.raises(capi.OtmbError) as e:
        D.periodic(S, dt=SR.MONTH, ncycle=3, ptol=0.0)
    assert e.value.name == "INVALID_ARG" and "ptol" in str(e.value)
    # lines on an operator without lines
    p, i, v = R.dominant(257)
    with api.DeviceOperator(_csc(257, p, i, v)) as E:
        Y = _start(257, 2, 122)
        Y0 = Y.copy(order="F")
        assert _periodic_c(E, Y, 257, 2, S=Y0, lds=257, precond=1, dt=2.0)[0] == 11 and np.array_equal(Y, Y0)
        with pytest.raises(capi.OtmbError) as e:
            E.periodic(Y0, dt=2.0, ncycle=3, precond="lines")
        assert e.value.name == "INVALID_ARG" and "lines" in str(e.value)
        Xe, ie = E.periodic(Y0, dt=2.0, ncycle=3)  # and it is usable afterwards
        assert ie.converged.all()
    D.select(0)
    _same_bits(D.mul(X0), before, "the operator after the refusals")
    Xs, info = D.periodic(S, dt=SR.MONTH, ncycle=3, d=d, precond="lines", rtol=RTOL)
    assert info.converged.all()


def test_maxcycles_is_a_reported_answer(oracle):
    """tiny_tripolar, maxcycles = 2 (and 6): OTMB_ERR_NOT_CONVERGED, every column MAXCYCLES, cycles <= maxcycles, and defect is what one
    further step cycle from the returned X measures (to the rounding of two orders of one sum of N squares)."""
    from otmb_amd import capi

    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    d = R.shift("age", N, nsurf)[0]
    S = _start(N, 2, 131)
    with _operator(N, *T, nxt=nxt) as D:
        kw = dict(dt=SR.MONTH, theta=1.0, first_slot=0, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines")
        G, _ = D.step(np.zeros_like(S), nsteps=12, source=S, **kw)
        for maxcycles in (2, 6):
            X, info = D.periodic(S, ncycle=12, ptol=PTOL, restart=30, maxcycles=maxcycles, **kw)
            print("maxcycles", maxcycles, info)
            assert info.status == 19 and info.reason == ("maxcycles", "maxcycles") and (info.cycles <= maxcycles).all() and not info.converged.any()
            if maxcycles == 2:
                msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
                assert msg == (f"{capi.lib().otmb_status_string(19).decode()}: periodic: 2 of 2 columns; the first is column 1: maxcycles after "
                               f"{int(info.cycles[0])} cycles, defect {info.defect[0]:.3e}"), msg
            FX, _ = D.step(X, nsteps=12, source=S, **kw)
            measured = np.linalg.norm(FX - X, axis=0) / np.linalg.norm(G, axis=0)
            assert np.allclose(info.defect, measured, rtol=N * 2.0 ** -52, atol=0.0), (info.defect, measured)
            if maxcycles == 6:
                assert (info.cycles == 6).all() and (info.defect < 1.0).all()  # g, four iterations, their verification
        assert D.slots == (3, 0)


def test_a_nan_source_column_stops_alone(small):
    """k = 3 with one NaN in column 1 of the source: that column stops (its first step cannot converge), OTMB_ERR_NOT_CONVERGED with the
    step's own text, and columns 0 and 2 have the bits, cycles and defects of a clean call on those two columns."""
    from otmb_amd import capi

    D, N, T, d, S7 = small
    S = np.asfortranarray(S7[:, :3].copy())
    S[5, 1] = np.nan
    kw = dict(dt=SR.MONTH, ncycle=3, theta=0.5, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=10)
    X, info = D.periodic(S, **kw)
    msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
    print(info, msg)
    assert info.status == 19 and info.reason[0] == info.reason[2] == "converged" and info.reason[1] in ("step_failed", "nonfinite"), info
    assert "(step 0, slot 2)" in msg, msg
    assert "; the step: " in msg and msg.split("; the step: ", 1)[1].endswith("(step 0, slot 2)"), msg
    assert not X[:, 1].any()  # (the start, zero, is what it keeps)
    clean, ic = D.periodic(S[:, [0, 2]], **kw)
    assert ic.converged.all()
    _same_bits(X[:, [0, 2]], clean, "the clean columns")
    _same_bits(info.defect[[0, 2]], ic.defect, "their defects")
    assert np.array_equal(info.cycles[[0, 2]], ic.cycles)
    assert D.slots == (3, 0)


def test_padded_device_arrays_have_the_compact_calls_bits():
    """solve_ref.dominant(257) with random lines, k = 5, otmb_op_periodic_dev on tensors of n + 3 (S) and n + 5 (X) rows, NaN in the input
    padding, the sentinel in the output padding: rows [:n] have the bits of the compact call (whose odd leading dimension takes the 8-byte
    path where the padded one takes the 16-byte path), the padding and S keep theirs."""
    from otmb_amd.device import DeviceAssembler
    from test_op_padded_dev import _System, _pad, _raw, _same

    n, k = 257, 5
    P = _System(DeviceAssembler(0).ctx, n, R.dominant(n), np.random.default_rng(13).uniform(0.0, 1.0, n), 0.5, k, nxt=LR.random_lines(n, 3))
    S0, X0 = _start(n, k, 141), _start(n, k, 142)

    def call(S, lds, X, ldx, use_x0, pc, adjoint):
        cyc, dft, why = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32)
        rc = P.lib.otmb_op_periodic_dev(P.h, adjoint, k, P.dd.data_ptr(), 2.0, 0.5, 4, FIRST, S.data_ptr(), lds, X.data_ptr(), ldx, use_x0, RTOL, MAXITER, pc,
                                        PTOL, 4, 200, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data)
        return rc, cyc, dft, why

    try:
        for use_x0, pc, adjoint in ((0, 1, 0), (1, 0, 1)):
            Sc, Xc = _pad(S0, 0, np.nan), _pad(X0 if use_x0 else np.full((n, k), SENTINEL), 0, SENTINEL)
            rc, cyc, dft, why = call(Sc, n, Xc, n, use_x0, pc, adjoint)
            print("compact", use_x0, pc, adjoint, rc, cyc.tolist(), dft.tolist())
            assert rc == 0 and (why == 0).all() and (dft <= PTOL).all()
            Sp, Xp = _pad(S0, 3, np.nan), _pad(X0 if use_x0 else np.full((n, k), SENTINEL), 5, SENTINEL)
            rcp, cycp, dftp, whyp = call(Sp, n + 3, Xp, n + 5, use_x0, pc, adjoint)
            assert rcp == 0 and np.array_equal(cycp, cyc) and np.array_equal(whyp, why)
            _same(dftp, dft, "defect")
            _same(Xp[:n], Xc, "rows [:n] of the padded call")
            assert (Xp[n:] == SENTINEL).all().item() and Sp[n:].isnan().all().item()
            _same(Sp[:n], S0, "S is not written")
            assert P.O.slots == (3, 0)
    finally:
        P.O.close()


def test_the_assemblers_route_has_the_operators_bits():
    """DeviceAssembler.periodic_tracers on three kept months of small_rho3d (the fixture of tests/test_step_assembler.py) against
    api.DeviceOperator.periodic over the same three value sets: X, cycles, defect and reason, bit for bit.  (The subject is the route; the
    bound maxcycles = 40 may or may not be reached, either answer must be the same.)"""
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
        asm.keep_slot(m, nslots=3)
        months.append(_host(asm)["T"])
    rng = np.random.default_rng(151)
    S = _start(N, 2, 152)
    d = rng.uniform(0.5e-7, 1.5e-7, N)  # a sink everywhere: without one Φ has the eigenvalue 1 (T conserves mass)
    Sd = torch.from_numpy(S).cuda().t().contiguous().t()
    kw = dict(dt=SR.MONTH, ncycle=3, theta=1.0, first_slot=1, rtol=1e-10, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=10, maxcycles=40)
    Xa, ia = asm.periodic_tracers(Sd, d=torch.from_numpy(d).cuda(), **kw)
    p, i, _ = months[0]
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, months[0][2])) as D:
        D.set_lines(asm.vertical_lines().cpu().numpy())
        D.set_slots(3)
        for m in range(1, 3):
            D.set_values(months[m][2], slot=m)
        Xo, io = D.periodic(S, d=d, **kw)
    print("assembler", ia, io)
    assert ia.status == io.status and ia.reason == io.reason and np.array_equal(ia.cycles, io.cycles) and (ia.cycles > 1).all()
    _same_bits(Xa.cpu().numpy(), Xo, "periodic_tracers")
    _same_bits(ia.defect, io.defect, "defect")
    with pytest.raises(ValueError, match="keep_slot"):
        asm.periodic_tracers(Sd, matrix="Tadv", **kw)
