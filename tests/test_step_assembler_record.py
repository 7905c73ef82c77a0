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
