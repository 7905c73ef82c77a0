"""CPU: the bookkeeping of DeviceAssembler.keep_slot / operator / step_tracers / forget_slots (device.py) with the resident operator
replaced by a stand-in that records what each slot was given.  What is checked is which slot every call writes: a year kept month by
month holds month m in slot m whether the record vouches for the pattern (a values-only fill) or not (a full write: the pattern is
compared with the copy keep_slot took); nothing refreshes or replaces an operator that has slots; another pattern raises and leaves them.
(tests/test_step_assembler.py runs the same protocol on the device against api.DeviceOperator.step.)"""
import pytest
import torch

from otmb_amd import device
from otmb_amd.device import DeviceAssembler

N, NNZ = 6, 9


class _Handle:
    value = 1


class _Op:
    """What device.Operator is to the assembler: slots of values over one pattern."""
    made = 0

    def __init__(self, ctx, m, n, cp, rv, nz):
        _Op.made += 1
        self.handle, self.nnz = _Handle(), NNZ
        self.vals, self.sel, self.writes = [nz[:NNZ].clone()], 0, []

    @property
    def slots(self):
        return len(self.vals), self.sel

    def set_lines(self, nxt):
        pass

    def set_slots(self, n):
        self.vals = self.vals[:n] + [self.vals[self.sel].clone() for _ in range(n - len(self.vals))]
        self.sel = self.sel if self.sel < n else 0

    def set_values_dev(self, nz, slot=None):
        slot = self.sel if slot is None else int(slot)
        assert 0 <= slot < len(self.vals)
        self.vals[slot] = nz[:NNZ].clone()
        self.writes.append(slot)

    def select(self, slot):
        assert 0 <= slot < len(self.vals)
        self.sel = int(slot)

    def step(self, X, **kw):
        return [v.clone() for v in self.vals], kw

    def close(self):
        self.handle = type("H", (), {"value": 0})()


class _Ctx:
    fills = 0

    def synchronize(self):
        pass

    def kept_t_pattern_fills(self):
        return self.fills


@pytest.fixture
def asm(monkeypatch):
    monkeypatch.setattr(device, "Operator", _Op)
    _Op.made = 0
    a = object.__new__(DeviceAssembler)
    a._init_state()
    a.ctx, a.N = _Ctx(), N
    a.vertical_lines = lambda: None
    a.out = {m: (torch.arange(1, N + 2), torch.arange(1, NNZ + 3), torch.zeros(NNZ + 2, dtype=torch.float64)) for m in device.MATS}
    a.nnz = [NNZ] * len(device.MATS)
    return a


def _build(a, month, vouched, pattern=None):
    """What a step of the assembler leaves behind for the operators: new values in place, the record told (_ops_written)."""
    a.out["T"][2][:] = float(month)
    if pattern is not None:
        a.out["T"][1][:NNZ] = pattern
    a._tpat_last, a._tpat_fills0 = vouched, a.ctx.fills
    if vouched:
        a.ctx.fills += 1
    a._ops_written(a.out, device.DeviceAssembler.KEPT if vouched else ())


def _months(op):
    return [float(v[0]) for v in op.vals]


@pytest.mark.parametrize("vouched", [True, False])
def test_a_year_kept_month_by_month(asm, vouched):
    for m in range(12):
        _build(asm, 100 + m, vouched and m > 0)
        op = asm.keep_slot(m, nslots=12)
        assert op.slots == (12, m)
        assert asm.operator("T") is op and op.writes[-1:] in ([], [m])  # (mul / solve after keep_slot write nothing more)
    assert _Op.made == 1 and _months(op) == [100.0 + m for m in range(12)]
    assert op.writes == list(range(1, 12))  # each month once, into its own slot (slot 0 had January from the plan)
    # a month built and not kept: nothing is written, operator() refuses, the tracers read the year as kept
    _build(asm, 999, vouched)
    with pytest.raises(ValueError, match="keep_slot"):
        asm.operator("T")
    vals, kw = asm.step_tracers(None, dt=1.0)
    assert [float(v[0]) for v in vals] == [100.0 + m for m in range(12)] and kw == {"dt": 1.0} and _Op.made == 1
    asm.keep_slot(3)
    assert _months(op) == [100.0, 101.0, 102.0, 999.0] + [104.0 + m for m in range(8)] and op.slots == (12, 3)
    assert asm.operator("T") is op


def test_another_pattern_raises_and_the_slots_stay(asm):
    for m in range(2):
        _build(asm, 100 + m, m > 0)
        op = asm.keep_slot(m, nslots=3)
    with pytest.raises(ValueError):
        asm.keep_slot(3)
    other = torch.arange(NNZ, 0, -1)
    for vouched in (False, True):  # (a full write of another pattern; and a record that cannot vouch stays unable to)
        _build(asm, 555, vouched, pattern=other)
        for call in (lambda: asm.keep_slot(2), lambda: asm.operator("T")):
            with pytest.raises(ValueError, match="forget_slots"):
                call()
        assert _Op.made == 1 and op.handle.value and _months(op) == [100.0, 101.0, 100.0] and op.slots == (3, 1)
    asm.nnz[0] = NNZ - 1  # (and a compacted T: another nnz)
    with pytest.raises(ValueError, match="forget_slots"):
        asm.keep_slot(2)
    asm.nnz[0] = NNZ
    asm.forget_slots()
    assert not op.handle.value
    with pytest.raises(ValueError, match="keep_slot"):
        asm.step_tracers(None, dt=1.0)
    op2 = asm.keep_slot(0)
    assert _Op.made == 2 and op2.slots == (1, 0) and _months(op2) == [555.0]


def test_one_slot_behaves_as_before(asm):
    """Without slots operator() refreshes the values when the pattern is vouched for and plans again when it is not."""
    _build(asm, 1, False)
    op = asm.operator("T")
    _build(asm, 2, True)
    assert asm.operator("T") is op and _months(op) == [2.0] and asm.op_reuses == 1
    _build(asm, 3, False)
    op3 = asm.operator("T")
    assert op3 is not op and not op.handle.value and _months(op3) == [3.0] and asm.op_replans == 2


# ---- which promises a call may make (_kept_ops) after an accepted call (_kept_written), on CPU tensors ------------------------------------
KEPT = DeviceAssembler.KEPT
K = sum(1 << device.MATS.index(m) for m in KEPT)  # the three operator bits
P, R = device.capi.KEPT_T_PATTERN, device.capi.KEPT_RHO
GRID = ("lwet3d", "lwet", "v3d", "thk", "area", "zt", "mlotst") + tuple(f"{w}{q}" for w in ("edge", "dist") for q in range(4))


def _grid_asm():
    """An assembler with a grid of CPU tensors and a stand-in context, and a five-matrix output set of its own."""
    f = lambda n=4: torch.zeros(n, dtype=torch.float64)
    i = lambda n=4: torch.zeros(n, dtype=torch.int64)
    a = object.__new__(DeviceAssembler)
    a._init_state()
    a.ctx, a.N = _Ctx(), N
    a.lwet3d, a.lwet, a.v3d, a.thk, a.area, a.zt, a.mlotst = i(), i(), f(), f(), f(), f(), f()
    a.edge, a.dist = [f() for _ in range(4)], [f() for _ in range(4)]
    a.kappa, a.rho = (500.0, 0.1, 1e-5), f()
    return a, {m: (i(N + 1), i(NNZ), f(NNZ)) for m in device.MATS}


@pytest.fixture
def kept(monkeypatch):
    monkeypatch.delenv("OTMB_KEPT", raising=False)
    return _grid_asm()


def _grid_tensor(a, name):
    return getattr(a, name[:4])[int(name[4])] if name[:4] in ("edge", "dist") else getattr(a, name)


def test_no_promise_before_anything_was_written(kept):
    a, out = kept
    assert a._kept_ops(out) == (0, ())


def test_every_promise_when_nothing_happened_since(kept):
    a, out = kept
    a._kept_written(out, ())
    assert a._kept_ops(out) == (K | P | R, KEPT)
    a._kept_written(out, KEPT)
    assert a._kept_ops(out) == (K | P | R, KEPT)
    assert a._kept_last == () and a._tpat_last is True  # (of the call being prepared, until _kept_written says it was accepted)
    a._kept_written(out, KEPT)
    assert a._kept_last == KEPT and a._kept_steady() == set(KEPT)


@pytest.mark.parametrize("q", [0, 1])
def test_an_edit_of_T_pattern_withdraws_the_pattern_alone(kept, q):
    a, out = kept
    a._kept_written(out, KEPT)
    out["T"][q].add_(0)
    assert a._kept_ops(out) == (K | R, KEPT) and a._tpat_last is False


@pytest.mark.parametrize("m,q", [("T", 2), ("Tadv", 0), ("Tadv", 1), ("Tadv", 2)])
def test_an_edit_of_T_values_or_of_Tadv_withdraws_nothing(kept, m, q):
    a, out = kept
    a._kept_written(out, KEPT)
    out[m][q].add_(0)
    assert a._kept_ops(out) == (K | P | R, KEPT)


@pytest.mark.parametrize("how", ["clone", "inplace"])
def test_another_rho_withdraws_rho_alone(kept, how):
    a, out = kept
    a._kept_written(out, KEPT)
    if how == "clone":
        a.rho = a.rho.clone()
    else:
        a.rho.add_(0)
    assert a._kept_ops(out) == (K | P, KEPT)


@pytest.mark.parametrize("m", KEPT)
@pytest.mark.parametrize("q", [0, 1, 2])
def test_an_edit_of_a_kept_operator_withdraws_everything(kept, m, q):
    a, out = kept
    a._kept_written(out, KEPT)
    out[m][q].add_(0)
    assert a._kept_ops(out) == (0, ())


@pytest.mark.parametrize("name", GRID)
def test_an_edit_of_a_grid_tensor_withdraws_everything(kept, name):
    a, out = kept
    a._kept_written(out, KEPT)
    _grid_tensor(a, name).add_(0)
    assert a._kept_ops(out) == (0, ())


def test_another_kappa_only_T_or_a_given_operator_withdraw_everything(kept):
    a, out = kept
    a._kept_written(out, KEPT)
    a.kappa = (1.0, 0.1, 1e-5)
    assert a._kept_ops(out) == (0, ())
    a.kappa = (500.0, 0.1, 1e-5)
    assert a._kept_ops(out) == (K | P | R, KEPT)
    a.only_T = True
    assert a._kept_ops(out) == (0, ())
    a.only_T = False
    assert a._kept_ops(out) == (K | P | R, KEPT)
    a.given = {"TκH": out["TκH"]}
    assert a._kept_ops(out) == (0, ())
    a.given = {}
    assert a._kept_ops(out) == (K | P | R, KEPT)


def test_a_call_with_a_given_operator_leaves_no_promise_behind(kept):
    a, out = kept
    a._kept_written(out, KEPT)
    a.given = {"TκH": out["TκH"]}
    a._kept_written(out, ())
    a.given = {}
    assert a._kept_ops(out) == (0, ())


def test_a_call_for_T_alone_leaves_no_promise_behind(kept):
    a, out = kept
    a.only_T = True
    a._kept_written(out, ())
    a.only_T = False
    assert a._kept_ops(out) == (0, ())


def test_another_output_set_with_equal_contents_gets_no_promise(kept):
    a, out = kept
    a._kept_written(out, KEPT)
    other = {m: tuple(t.clone() for t in out[m]) for m in device.MATS}
    assert a._kept_ops(other) == (0, ())
    assert a._kept_ops(out) == (K | P | R, KEPT)  # (asking is no edit)


def test_forget_kept_withdraws_everything(kept):
    a, out = kept
    a._kept_written(out, KEPT)
    a._forget_kept()
    assert a._kept_last == () and a._tpat_last is False and a._kept_steady() == set()
    assert a._kept_ops(out) == (0, ())
    assert a._kept_last == () and a._tpat_last is False


def test_OTMB_KEPT_0_makes_no_promise(monkeypatch):
    monkeypatch.setenv("OTMB_KEPT", "0")
    a, out = _grid_asm()
    a._kept_written(out, ())
    assert a._kept_ops(out) == (0, ()) and a._kept_steady() == set()


def test_two_assemblers_share_no_state(kept):
    a, out = kept
    b, out_b = _grid_asm()
    a._kept_written(out, KEPT)
    a.given = {"TκH": out["TκH"]}
    assert b._kept_ops(out_b) == (0, ()) and b._kept_steady() == set() and not getattr(b, "given", None)
