"""DeviceAssembler.keep_slot / step_tracers / forget_slots (device.py): months built by asm.step and kept one by one are the slots a tracer
run cycles through.  keep_slot writes its slot ALONE (no other slot changes, whichever way the operator's record stood), step_tracers has
the bits of api.DeviceOperator.step on the same value sets, asm.mul goes on reading the month just built, and a month that cannot share
the slots' pattern is refused with the slots left as they are."""
import numpy as np
import pytest

import step_ref as SR
from spmv_ref import bits, spmv_ref

pytestmark = pytest.mark.gpu

MONTHS = 3


def _same_bits(a, b, what):
    assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), what


@pytest.mark.parametrize("vouched", [True, False])
def test_months_kept_one_by_one_step_like_an_operator_over_the_same_values(monkeypatch, vouched):
    """small_rho3d (N = 6962), three months through asm.step + keep_slot(m, nslots=3), then a fourth built and NOT kept.  vouched: the
    library keeps T's pattern from the second month on (the record holds); not vouched (OTMB_KEPT=0: every month is written in full): the
    pattern is compared with the copy keep_slot took.  Either way: after every keep_slot asm.mul("T") is the product with that month; slot m
    holds month m for every m at the end (select + mul against the restatement on the downloaded values); step_tracers (θ = 1 and 0.5,
    lines, 7 steps from slot 2, k = 3) equals DeviceOperator.step over the same three value sets bit for bit, iterations included."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _fields, _host, _pair

    if not vouched:
        monkeypatch.setenv("OTMB_KEPT", "0")
    g, gm, asm, other, umo, vmo, fill = _pair("small_rho3d")
    del other
    N = asm.N
    rng = np.random.default_rng(31)
    x = rng.standard_normal(N)
    xd = torch.from_numpy(x).cuda()
    fields = _fields(umo, vmo, MONTHS + 1, seed=5)
    months = []
    for m in range(MONTHS):
        asm.step(*fields[m], fill)
        op = asm.keep_slot(m, nslots=MONTHS)
        assert op.slots == (MONTHS, m)
        months.append(_host(asm)["T"])
        _same_bits(asm.mul("T", xd).cpu().numpy(), spmv_ref(N, N, *months[m], x), ("the month just kept", m))
    p, i, _ = months[0]
    assert all(np.array_equal(h[0], p) and np.array_equal(h[1], i) for h in months)
    assert len({h[2].tobytes() for h in months}) == MONTHS  # (three different value sets: a slot holding another month's would show)
    assert asm.op_replans == 1  # (one plan, at the first keep_slot; the later months moved values only)
    # a month built and not kept: no slot is written, mul has no slot to put it in and says so, the tracers step through what was kept
    asm.step(*fields[MONTHS], fill)
    with pytest.raises(ValueError, match="keep_slot"):
        asm.mul("T", xd)
    X0 = np.ones((N, 3), order="F")
    X0[:, 1:] = rng.standard_normal((N, 2))
    S = np.asfortranarray(rng.standard_normal((N, 3)) * 1e-7)
    Xd, Sd = (torch.from_numpy(a).cuda().t().contiguous().t() for a in (X0, S))
    nxt = asm.vertical_lines().cpu().numpy()
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, months[0][2])) as D:
        D.set_lines(nxt)
        D.set_slots(MONTHS)
        for m in range(1, MONTHS):
            D.set_values(months[m][2], slot=m)
        for theta in (1.0, 0.5):
            kw = dict(dt=SR.MONTH, theta=theta, nsteps=7, first_slot=2, rtol=1e-10, maxiter=5000, precond="lines")
            Xa, ia = asm.step_tracers(Xd, source=Sd, **kw)
            Xo, io = D.step(X0, source=S, **kw)
            print("vouched", vouched, "theta", theta, "iterations", io.iterations.tolist())
            assert ia.steps_done == io.steps_done == 7 and np.array_equal(ia.iterations, io.iterations)
            _same_bits(Xa.cpu().numpy(), Xo, ("step_tracers", theta))
            _same_bits(ia.relres, io.relres, ("relres", theta))
    op = asm._ops["T"].op
    assert op.slots == (MONTHS, MONTHS - 1)
    for m in range(MONTHS):  # every slot still holds its own month
        op.select(m)
        _same_bits(op.mul(xd).cpu().numpy(), spmv_ref(N, N, *months[m], x), ("slot", m))
    # keeping the fourth month into slot 0 replaces January alone
    asm.keep_slot(0)
    h = _host(asm)["T"]
    _same_bits(asm.mul("T", xd).cpu().numpy(), spmv_ref(N, N, *h, x), "slot 0 again")
    op.select(1)
    _same_bits(op.mul(xd).cpu().numpy(), spmv_ref(N, N, *months[1], x), "slot 1 untouched")


def test_a_month_with_another_pattern_is_refused_and_the_slots_stay():
    """κH = 0 with centred weights (tests/test_kept_t_pattern.py): the third month has exact cancellations, so its T is compacted to fewer
    entries.  keep_slot raises, the three slots and their values are as they were; forget_slots drops them and the month is kept in a new
    operator.  A slot outside the operator's is refused before anything changes."""
    import torch

    from helpers import make_case
    from test_kept_ops import MATS, _host, _pair
    from test_kept_t_pattern import _cancel_fields

    g0, _ = make_case("small_rho3d")
    g, gm, asm, other, umo, vmo, fill = _pair("small_rho3d", kappa=(0.0, g0.kappaVML, g0.kappaVdeep), upwind=False)
    del other
    N = asm.N
    fields = _cancel_fields(umo, vmo, 3, {2}, seed=42)
    x = np.random.default_rng(3).standard_normal(N)
    xd = torch.from_numpy(x).cuda()
    kept = []
    for m in range(2):
        asm.step(*fields[m], fill)
        op = asm.keep_slot(m, nslots=3)
        kept.append(_host(asm)["T"])
    with pytest.raises(ValueError):
        asm.keep_slot(3)
    assert op.slots == (3, 1)
    asm.step(*fields[2], fill)
    assert asm.nnz[MATS.index("T")] < len(kept[0][2])  # (the cancellations compacted T)
    with pytest.raises(ValueError, match="forget_slots"):
        asm.keep_slot(2)
    assert op.slots == (3, 1) and asm._ops["T"].op is op
    for m, h in enumerate((kept[0], kept[1], kept[0])):  # (growing copied the selected slot: the third holds the first month)
        op.select(m)
        _same_bits(op.mul(xd).cpu().numpy(), spmv_ref(N, N, *h, x), ("slot", m))
    asm.forget_slots()
    assert not op.handle.value
    op2 = asm.keep_slot(0)
    assert op2.slots == (1, 0)
    _same_bits(asm.mul("T", xd).cpu().numpy(), spmv_ref(N, N, *_host(asm)["T"], x), "after forget_slots")
