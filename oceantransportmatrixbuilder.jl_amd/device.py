"""Device-resident driver of the hot path: torch owns the HBM buffers and the stream, the C ABI
(`*_dev` entry points) does the work.  Used by bench.py, the GPU tests and smoke(); a Julia
caller with device-resident data (AMDGPU.jl ROCArrays) would call the same `_dev` symbols.

All arrays are flat torch tensors whose memory is Julia's column-major (nx,ny,nz) layout.
"""
import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import capi
from .capi import HDIRS, MATS, PHI_ORDER
from .operator_calls import OperatorCalls

# the library reads OTMB_KEPT_HTAB once per process (the first kept fill): what it will find, for accounting before that fill
_KEPT_HTAB_ON = os.environ.get("OTMB_KEPT_HTAB", "1")[:1] != "0"
_KEPT_TPAT_ON = os.environ.get("OTMB_KEPT_TPAT", "1")[:1] != "0"  # (likewise OTMB_KEPT_TPAT: T's values-only fills)


def _flat(a, dtype=np.float64):
    return np.asfortranarray(a, dtype=dtype).ravel(order="F")


def _col_major(t, rows):
    """(tensor, leading dimension) of a 1-D or 2-D float64 device tensor with unit row stride (a column-major matrix, or a row slice of
    one); anything else is copied into that layout."""
    if t.dtype != torch.float64:
        raise ValueError("float64 tensors are required")
    if t.dim() == 1:
        t = t if t.stride(0) == 1 else t.contiguous()
        return t, max(rows, 1)
    if t.stride(0) != 1 or (t.shape[1] > 1 and t.stride(1) < rows):
        t = t.t().contiguous().t()
    return t, max(t.stride(1) if t.shape[1] > 1 else rows, rows, 1)


def _on_device(t, device, what):
    """A host tensor's pointer handed to a kernel would fault the device: refuse anything that is not on the operator's GPU."""
    if not torch.is_tensor(t) or not t.is_cuda or t.device.index != device:
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what} must be a tensor on cuda:{device} (got {where})")


class Operator(OperatorCalls):
    """A resident sparse operator over device CSC arrays (otmb_op_create_dev): Y = α·A·X + β·Y and α·Aᵀ·X + β·Y on torch tensors, bit for
    bit SparseArrays' 5-argument mul! (api.DeviceOperator states the contract).  The operator owns device copies of the matrix;
    set_values_dev refreshes the values for the same pattern.  DeviceAssembler.operator() hands these out over its resident results.
    add_matrix, precondition, solve, observe, step and periodic are OperatorCalls' over the tensor hooks below (the `_dev` exports): a column-major
    tensor, or a row slice of one, is passed uncopied with its parent's leading dimension; results are new tensors."""

    _suffix = "_dev"

    def __init__(self, ctx, m, n, colptr, rowval, nzval):
        self.ctx, self.lib = ctx, capi.lib()
        self._h = C.c_void_p()
        self.device = int(ctx.device)
        for t, what in ((colptr, "colptr"), (rowval, "rowval"), (nzval, "nzval")):
            _on_device(t, self.device, what)
        self.ctx.check(self.lib.otmb_op_create_dev(self.ctx.handle, int(m), int(n), colptr.data_ptr(), rowval.data_ptr(), nzval.data_ptr(),
                                                   C.byref(self._h)))
        mm, nn, z = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.otmb_op_info(self._h, C.byref(mm), C.byref(nn), C.byref(z)))
        self.shape, self.nnz = (int(mm.value), int(nn.value)), int(z.value)

    @property
    def handle(self):
        return self._h

    # OperatorCalls' arrays: float64 tensors on this operator's GPU
    def _live(self):
        if not self._h.value:
            raise ValueError("operator is closed")

    def _library(self):
        return self.lib

    def _array(self, a, what):
        _on_device(a, self.device, what)
        return a

    def _matrix(self, a, rows):
        return _col_major(a, rows)

    def _ptr(self, a):
        return None if a is None else a.data_ptr()

    def _zeros(self, shape, order="F"):
        dev = torch.device("cuda", self.device)
        if order == "C" or len(shape) == 1:
            return torch.zeros(shape, dtype=torch.float64, device=dev)
        rows, k = shape
        return torch.zeros(k * max(rows, 1), dtype=torch.float64, device=dev).as_strided((rows, k), (1, max(rows, 1)))

    def _assign(self, X, a):
        X.copy_(a)

    def _check_d(self, d, want, what):
        if d.dtype != torch.float64 or tuple(d.shape) != want:
            raise capi.OtmbError(11, "DimensionMismatch: d must be " + (f"{want[0]} float64 values" if len(want) == 1 else
                                                                       f"float64 of {what}'s shape {want}, not {tuple(d.shape)}"))

    # ... and of the domain calls (submatrix, take_values, to_csc, lines: OperatorCalls'): masks become index tensors on the device
    def _selection(self, s, limit, what):
        if not torch.is_tensor(s):
            s = torch.as_tensor(np.asarray(s), device=torch.device("cuda", self.device))
        _on_device(s, self.device, what)
        if s.dtype == torch.bool:
            if tuple(s.shape) != (limit,):
                raise capi.OtmbError(11, f"DimensionMismatch: {what} mask of {tuple(s.shape)}, expected {(limit,)}")
            return torch.nonzero(s).flatten() + 1
        if s.dim() != 1 or (s.is_floating_point() and s.numel() > 0) or s.is_complex():
            raise capi.OtmbError(11, f"invalid argument: {what} must be a boolean mask or a 1-D tensor of integers, got {s.dtype} of {tuple(s.shape)}")
        return s.to(torch.int64).contiguous() + 1

    def _empty(self, n, dtype):
        return torch.empty(n, dtype=getattr(torch, dtype), device=torch.device("cuda", self.device))

    def _csc(self, cp, rv, nz):
        return cp, rv, nz

    def _csc_arrays(self, B):
        cp, rv, nz = B
        for t, what, dtype in ((cp, "B's colptr", torch.int64), (rv, "B's rowval", torch.int64), (nz, "B's nzval", torch.float64)):
            _on_device(t, self.device, what)
            if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
                raise capi.OtmbError(11, f"invalid argument: {what} must be a contiguous 1-D {dtype} tensor")
        if cp.numel() != self.shape[1] + 1 or rv.numel() != nz.numel():
            raise capi.OtmbError(11, f"DimensionMismatch: operator of {self.shape}, B's colptr of {cp.numel()}, rowval of {rv.numel()}, nzval of {nz.numel()}")
        return cp, rv, nz

    def _adopt(self, h):
        D = Operator.__new__(Operator)
        D.ctx, D.lib, D._h, D.device = self.ctx, self.lib, h, self.device
        D.shape, D.nnz = self._info(h)
        return D

    def set_values_dev(self, nzval, slot=None):
        """New values from a device tensor for the selected slot, or for slot `slot` (set_slots)."""
        _on_device(nzval, self.device, "nzval")
        if nzval.dtype != torch.float64 or not nzval.is_contiguous() or nzval.numel() < self.nnz:
            raise ValueError(f"nzval: a contiguous float64 tensor of at least {self.nnz} entries is required")
        if slot is None:
            self.ctx.check(self.lib.otmb_op_set_values_dev(self._h, nzval.data_ptr(), self.nnz))
        else:
            self.ctx.check(self.lib.otmb_op_set_values_slot_dev(self._h, int(slot), nzval.data_ptr(), self.nnz))

    set_values = set_values_dev

    def set_slots(self, n):
        """n >= 1 value slots over the one pattern (otmb_op_set_slots; api.DeviceOperator.set_slots)."""
        self.ctx.check(self.lib.otmb_op_set_slots(self._h, int(n)))

    def select(self, slot):
        """mul, solve and precondition read slot `slot` from now on (a pointer switch)."""
        self.ctx.check(self.lib.otmb_op_select_slot(self._h, int(slot)))

    def combine_slots(self, weights, dst):
        """Slot dst = Σ_s weights[s]·(slot s), enqueued on the context's stream (otmb_op_combine_slots_dev; api.DeviceOperator.combine_slots).
        weights: host values, one per slot."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (self.slots[0],):
            raise capi.OtmbError(11, f"DimensionMismatch: weights of {w.shape}, expected {(self.slots[0],)}")
        self.ctx.check(self.lib.otmb_op_combine_slots_dev(self._h, w.ctypes.data, int(dst)))

    @property
    def slots(self):
        """(number of slots, the selected slot)."""
        n, sel = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.lib.otmb_op_slots(self._h, C.byref(n), C.byref(sel)))
        return int(n.value), int(sel.value)

    def mul(self, X, *, alpha=1.0, beta=0.0, Y=None, adjoint=False):
        """X: 1-D or 2-D (rows x k, column-major) float64 device tensor; Y: None (a new tensor; β must be 0) or a tensor of the result's
        shape, updated in place.  Enqueued on the context's stream; nothing travels to the host."""
        self._live()
        _on_device(X, self.device, "X")
        if Y is not None:
            _on_device(Y, self.device, "Y")
        m, n = self.shape
        rx, ry = (m, n) if adjoint else (n, m)
        if X.dim() not in (1, 2) or X.shape[0] != rx:
            raise capi.OtmbError(11, f"DimensionMismatch: {'Aᵀ' if adjoint else 'A'} of {(ry, rx)} times X of {tuple(X.shape)}")
        k = 1 if X.dim() == 1 else X.shape[1]
        oshape = (ry,) if X.dim() == 1 else (ry, k)
        if Y is None:
            if beta != 0:
                raise ValueError("beta != 0 needs Y")
            Y = torch.empty(ry, dtype=torch.float64, device=X.device) if X.dim() == 1 else \
                torch.empty_strided((ry, k), (1, max(ry, 1)), dtype=torch.float64, device=X.device)
        if tuple(Y.shape) != oshape:
            raise capi.OtmbError(11, f"DimensionMismatch: Y of {tuple(Y.shape)}, expected {oshape}")
        Xc, ldx = _col_major(X, rx)
        Yc, ldy = _col_major(Y, ry)
        self.ctx.check(self.lib.otmb_op_mul_dev(self._h, int(bool(adjoint)), k, Xc.data_ptr(), ldx, Yc.data_ptr(), ldy, float(alpha), float(beta)))
        if Yc.data_ptr() != Y.data_ptr():
            Y.copy_(Yc)
        return Y

    def set_lines(self, next):
        """The lines of the "lines" preconditioner (otmb_op_set_lines_dev): a contiguous int64 device tensor of n entries, next[i] the 1-based
        successor of unknown i + 1 on its line or 0; None clears them.  Copied: the tensor may go afterwards."""
        self._live()
        if next is None:
            self.ctx.check(self.lib.otmb_op_set_lines_dev(self._h, None))
            return
        _on_device(next, self.device, "next")
        if next.dtype != torch.int64 or tuple(next.shape) != (self.shape[1],):
            raise capi.OtmbError(11, f"DimensionMismatch: next must be {self.shape[1]} int64 values")
        next = next.contiguous()
        self.ctx.check(self.lib.otmb_op_set_lines_dev(self._h, next.data_ptr()))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.otmb_op_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Snapshot:
    """The single definition of "unchanged since": `same` tensors recorded by identity (a weak reference: a recycled address is another
    tensor) and by (data_ptr, _version) -- any in-place torch op bumps _version; `also` tensors by (data_ptr, _version) alone; `values`
    by equality.  The kept promises and the operator records are snapshots, compared with what a call is about to be handed."""
    __slots__ = ("refs", "key")

    def __init__(self, same, also=(), values=()):
        self.refs = [weakref.ref(t) for t in same]
        self.key = self._key(same, also, values)

    @staticmethod
    def _key(same, also, values):
        return tuple((t.data_ptr(), t._version) for t in (*same, *also)) + tuple(values)

    def same_objects(self, same):  # (the recorded tensors themselves, whatever torch did to them since)
        return len(same) == len(self.refs) and all(r() is t for r, t in zip(self.refs, same))

    def matches(self, same, also=(), values=()):
        return self.same_objects(same) and self.key == self._key(same, also, values)


@dataclass
class OpRecord:
    """A resident operator over one of the assembler's result matrices and what is known of that result since the operator was planned."""
    op: object
    snapshot: _Snapshot = None  # the result's (colptr, rowval) as planned
    nzv: _Snapshot = None  # the result's (nzval,) as the operator last read it
    ok: bool = True  # every call since the plan left the pattern in place (_ops_written)
    dirty: bool = False  # the values were written since the operator read them
    pattern: tuple = None  # keep_slot's copy of (colptr, rowval[:nnz]): compared where `ok` cannot vouch


class DeviceAssembler:
    """Holds one grid (gridmetrics + indices + parameters) in HBM and assembles transport matrices
    for successive (umo, vmo) fields -- the TMIP workflow of building T for many time slices."""

    def __init__(self, device=0):
        self._init_state()
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceAssembler needs a GPU (no CPU fallback)")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.ctx = capi.Context(device)
        self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self.lib = capi.lib()

    def _init_state(self):
        """Every attribute the bookkeeping reads, at its "nothing yet" (tests that make an assembler without a GPU call this, not __init__)."""
        # grid (set_grid*, makeindices; _wetflags_version: wet3d._version when wetflags was folded): another grid forgets all but the counters
        self.shape = self.nx = self.ny = self.nz = self.G = self.N = self.topology = None
        self.v3d = self.thk = self.area = self.zt = self.mlotst = self.z3d = None
        self.edge, self.dist, self.dist_edge = [], [], []
        self.rho, self.rho_scalar, self.kappa, self.upwind = None, 0.0, None, True
        self.lwet3d = self.lwet = self.wet3d = self.wetflags = self.count_tables = self._wetflags_version = None
        # given operators (set_given): name -> (colptr, rowval, nzval), what the library's verdicts on them were keyed to; T alone (extension)
        self.given, self._given_key, self.only_T = {}, None, False
        # fluxes and mask (facefluxes_async, step_fused_async); _mask_key: the _phi_key the push mask and the tile counts describe, or None
        self.phi = self.push_mask = self.phi_top = self._mask_key = None
        # facefluxes also accumulates the tile counts of the transportmatrix that follows (otmb_facefluxes_counts_dev); False: the plain
        # kernel + the whole push mask + a counting pass, as before round 5 (A/B, and tests that look at the mask itself)
        self.count_in_ff = os.environ.get("OTMB_COUNT_IN_FF", "1") != "0"
        # pipeline sequence (_note, finish): the asynchronous calls not yet drained, each kind's numbers in the one sequence
        self._seq, self._ff_pending, self._ff_seq, self._tm_seq, self._ff_seq_drained = 0, 0, [], [], []
        # results: the output set of the last call, its capacities when made by new_output_set (None: sized by fill()), nnz, the two-phase plan
        self.out, self._out_cap, self.nnz, self._plan_kept = None, None, None, (None, ())
        # kept promises (_kept_ops / _kept_written): snapshots taken when a call was accepted, None: no promise; what the last call promised
        self._kept_on = os.environ.get("OTMB_KEPT", "1") != "0"  # (OTMB_KEPT=0: A/B)
        self._kept = self._tpat = self._rho_kept = None
        self._kept_last, self._tpat_last, self._tpat_fills0 = (), False, None
        # resident operators (operator, keep_slot): matrix name -> OpRecord, the output set the last accepted call wrote
        self._ops, self._op_last_out = {}, None
        # counters: operators handed out again, operators planned
        self.op_reuses = self.op_replans = 0

    def _t(self, a, dtype=np.float64):
        h = torch.from_numpy(_flat(a, dtype))
        d = self._empty(h.numel(), h.dtype)
        d.copy_(h)
        return d

    def _empty(self, n, dtype):
        """Device array of n elements (tools/placement_alloc.py overrides this for the placement experiments)."""
        return torch.empty(n, dtype=dtype, device=self.device)

    # ---- grid ---------------------------------------------------------------------------------
    def set_grid(self, gridmetrics, mlotst, rho, kappaH=500.0, kappaVML=0.1, kappaVdeep=1.0e-5, upwind=True):
        gm = gridmetrics
        self.shape = tuple(int(x) for x in gm["v3D"].shape)
        self.nx, self.ny, self.nz = self.shape
        self.G = self.nx * self.ny * self.nz
        t = gm["gridtopology"]
        self.topology = int(t["kind"]) if isinstance(t, dict) else int(t)
        self.v3d = self._t(gm["v3D"])
        self.thk = self._t(gm["thkcello"])
        self.edge = [self._t(gm["edge_length_2D"][d]) for d in HDIRS]
        self.dist = [self._t(gm["distance_to_neighbour_2D"][d]) for d in HDIRS]
        self.area = self._t(gm["area2D"])
        self.zt = self._t(gm["zt"])
        self.mlotst = self._t(mlotst)
        self.rho = None if np.ndim(rho) == 0 else self._t(rho)
        self.rho_scalar = float(rho) if np.ndim(rho) == 0 else 0.0
        self.kappa = (float(kappaH), float(kappaVML), float(kappaVdeep))
        self.upwind = bool(upwind)
        self.makeindices()

    def set_grid_tensors(self, *, shape, topology, v3d, thkcello, edge_length, dist_nbr, area2d, zt, mlotst, rho,
                         kappaH=500.0, kappaVML=0.1, kappaVdeep=1.0e-5, upwind=True):
        """Grid whose arrays already live on this GPU (flat float64 tensors in Julia's column-major order; edge_length /
        dist_nbr: four (nx*ny) tensors in OTMB_DIR_* order west, east, south, north; rho: tensor or number).  Nothing
        is copied: the caller keeps the tensors alive through this object."""
        self.shape = tuple(int(x) for x in shape)
        self.nx, self.ny, self.nz = self.shape
        self.G = self.nx * self.ny * self.nz
        self.topology = int(topology)
        self.v3d, self.thk = v3d, thkcello
        self.edge, self.dist = list(edge_length), list(dist_nbr)
        self.area, self.zt, self.mlotst = area2d, zt, mlotst
        self.rho = rho if torch.is_tensor(rho) else None
        self.rho_scalar = 0.0 if torch.is_tensor(rho) else float(rho)
        for t in (self.v3d, self.thk, *self.edge, *self.dist, self.area, self.zt, self.mlotst) + ((self.rho,) if self.rho is not None else ()):
            if t.device != self.device or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("set_grid_tensors: contiguous float64 tensors on this assembler's device are required")
        if self.v3d.numel() != self.G or self.thk.numel() != self.G or self.zt.numel() != self.nz:
            raise ValueError("set_grid_tensors: array sizes do not match shape")
        self.kappa = (float(kappaH), float(kappaVML), float(kappaVdeep))
        self.upwind = bool(upwind)
        self.makeindices()

    def set_grid_from_raw(self, *, areacello, volcello, lon, lat, lev, lon_vertices, lat_vertices, mlotst, rho,
                          kappaH=500.0, kappaVML=0.1, kappaVdeep=1.0e-5, upwind=True):
        """makegridmetrics on the device (otmb_makegridmetrics_dev): the raw CMIP arrays go up once, every derived
        array stays in HBM.  Host work is limited to the vertex permutation and the topology test."""
        from . import gridtopology as gt
        from ._nt import data_and_props
        from .gridmetrics import vertexpermutation

        area, ap = data_and_props(areacello)
        vol, vp = data_and_props(volcello)
        area = np.asfortranarray(area, dtype=np.float64)
        vol = np.asfortranarray(vol, dtype=np.float64)
        lonv = np.asfortranarray(data_and_props(lon_vertices)[0], dtype=np.float64)
        latv = np.asfortranarray(data_and_props(lat_vertices)[0], dtype=np.float64)
        perm = vertexpermutation(lonv, latv)
        topo = gt.getgridtopology(lonv[perm], latv[perm])
        self.shape = tuple(int(x) for x in vol.shape)
        self.nx, self.ny, self.nz = self.shape
        self.G, P = self.nx * self.ny * self.nz, self.nx * self.ny
        self.topology = topo
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=self.device)
        self.area, self.v3d, self.thk, self.z3d = f64(P), f64(self.G), f64(self.G), f64(self.G)
        self.edge, self.dist_edge, self.dist = [f64(P) for _ in range(4)], [f64(P) for _ in range(4)], [f64(P) for _ in range(4)]
        d_vol, d_area = self._t(vol), self._t(area)
        d_lon, d_lat = self._t(np.asarray(data_and_props(lon)[0])), self._t(np.asarray(data_and_props(lat)[0]))
        d_lonv, d_latv = self._t(lonv), self._t(latv)
        pa = (C.c_int32 * 4)(*perm)
        self.ctx.check(self.lib.otmb_makegridmetrics_dev(
            self.ctx.handle, d_vol.data_ptr(), d_area.data_ptr(), float(ap.get("_FillValue", np.nan)),
            float(vp.get("_FillValue", np.nan)), d_lon.data_ptr(), d_lat.data_ptr(), d_lonv.data_ptr(), d_latv.data_ptr(),
            C.byref(pa), self.nx, self.ny, self.nz, topo, self.area.data_ptr(), self.v3d.data_ptr(), self.thk.data_ptr(),
            self.z3d.data_ptr(), C.byref(capi.ptr_array(4, [t.data_ptr() for t in self.edge])),
            C.byref(capi.ptr_array(4, [t.data_ptr() for t in self.dist_edge])),
            C.byref(capi.ptr_array(4, [t.data_ptr() for t in self.dist]))))
        self.ctx.synchronize()
        self.zt = self._t(np.asarray(data_and_props(lev)[0]))
        self.mlotst = self._t(mlotst)
        self.rho = None if np.ndim(rho) == 0 else self._t(rho)
        self.rho_scalar = float(rho) if np.ndim(rho) == 0 else 0.0
        self.kappa = (float(kappaH), float(kappaVML), float(kappaVdeep))
        self.upwind = bool(upwind)
        self.makeindices()

    # ---- operators the caller passes (transportmatrix's Tadv = / TκH = / TκVML = / TκVdeep = keywords, src/matrixbuilding.jl:133-143) ----
    def set_given(self, **ops):
        """ops: name -> (colptr, rowval, nzval) device tensors (int64, int64, float64; rowval / nzval exactly nnz long) or None.  A passed
        operator is not built (otmb_tm_args.given): a TκH / TκVdeep with the rows the library derives for this grid is neither written nor
        counted -- its values are re-derived in registers or read where they lie (those of another κ included: ctx.given_state(m) == 3);
        any other matrix makes T a device sparse add (two-phase protocol only: transportmatrix(); the asynchronous calls raise
        GIVEN_FOREIGN)."""
        given = dict(self.given)
        for name, triple in ops.items():
            if name not in MATS[1:]:
                raise ValueError(f"{name}: not an operator of transportmatrix")
            if triple is None:
                given.pop(name, None)
                continue
            cp, rv, nz = (t.contiguous() for t in triple)
            if cp.dtype != torch.int64 or rv.dtype != torch.int64 or nz.dtype != torch.float64 or cp.numel() != self.N + 1 or rv.numel() != nz.numel():
                raise ValueError(f"{name}: (colptr int64 [N + 1], rowval int64 [nnz], nzval float64 [nnz]) device tensors are required")
            given[name] = (cp, rv, nz)
        self.given = given
        self._given_key = None
        self._forget_kept()  # (a given operator's slot is left unwritten: the library drops its record too)

    def _given_versions(self):
        ts = [self.lwet3d, self.lwet, self.v3d, self.thk, self.area, self.zt, *self.edge, *self.dist]
        for name in MATS[1:]:
            ts += list(self.given.get(name, ()))
        return tuple((t.data_ptr(), t._version) for t in ts) + tuple(self.kappa)

    def makeindices(self):
        """otmb_makeindices_dev on the resident v3D (src/matrixbuilding.jl:10-24)."""
        self._mask_key = None
        self._forget_kept()
        self.given, self._given_key = {}, None  # (operators of another grid)  # (fluxes of an earlier facefluxes call no longer come with counts / a mask for THESE indices)
        self.lwet3d = self._empty(self.G, torch.int64)
        self.lwet = self._empty(self.G, torch.int64)
        self.wet3d = torch.empty(self.G, dtype=torch.uint8, device=self.device)
        n = C.c_int64(0)
        self.ctx.check(self.lib.otmb_makeindices_dev(self.ctx.handle, self.v3d.data_ptr(), self.nx, self.ny, self.nz,
                                                     self.lwet3d.data_ptr(), self.lwet.data_ptr(),
                                                     self.wet3d.data_ptr(), C.byref(n)))
        self.N = int(n.value)
        # the five wet bytes nofluxboundaries! reads per cell and level, folded into one (otmb_wetflags_dev): once per grid
        self.wetflags = torch.empty(self.G, dtype=torch.uint8, device=self.device)
        self._wetflags_version = None
        self._fold_wet_mask(tables=True)
        return self.N

    def _fold_wet_mask(self, tables):
        """Fold wet3d into wetflags again when it is new or was edited in place since the last fold (tests do); tables: the count tables are
        then built again as well.  makeindices and step_fused_async ask for that, facefluxes_async does not and never did: whether its counts
        should follow an edited mask is an open question, and the asymmetry is left as it was found."""
        if self.wet3d._version == self._wetflags_version:
            return
        self.ctx.check(self.lib.otmb_wetflags_dev(self.ctx.handle, self.wet3d.data_ptr(), self.nx, self.ny, self.nz, self.topology,
                                                  self.wetflags.data_ptr()))
        self._wetflags_version = self.wet3d._version
        if tables:
            self._count_tables()

    def _count_tables(self):
        """Counts in facefluxes (otmb_facefluxes_counts_dev), once per grid: the wet rank at which every 64-cell wave segment starts and the
        per-tile row counts that depend on the wet mask alone."""
        nb = int(self.lib.otmb_count_tables_bytes(self.ctx.handle, self.nx, self.ny, self.nz, self.N))
        self.count_tables = torch.empty(max((nb + 7) // 8, 1), dtype=torch.int64, device=self.device)
        self.ctx.check(self.lib.otmb_count_tables_dev(self.ctx.handle, self.lwet3d.data_ptr(), self.lwet.data_ptr(), self.wetflags.data_ptr(),
                                                      self.N, self.nx, self.ny, self.nz, self.topology, self.count_tables.data_ptr()))

    # ---- per time slice -----------------------------------------------------------------------
    def facefluxes(self, umo, vmo, fill):
        """umo/vmo: flat device tensors (float64 or float32).  Returns the six ϕ tensors (reused).  Raises the
        reference's "all values missing" assertion (velocities.jl:199-200) like otmb_facefluxes_dev."""
        phi = self.facefluxes_async(umo, vmo, fill)
        self._check_missing()
        return phi

    def facefluxes_async(self, umo, vmo, fill):
        """Same kernel, no host round trip: the "all values missing" assertion is evaluated by finish().  The
        kernel also writes the push mask of these fluxes (include/otmb.h), which lets the counting pass of the
        following transportmatrix skip the six ϕ arrays."""
        if self.phi is None:
            self.phi = [self._empty(self.G, torch.float64) for _ in range(6)]
            self.push_mask = self._empty(self.G, torch.int16)
        ptrs = capi.ptr_array(6, [p.data_ptr() for p in self.phi])
        self._mask_key = None
        self._note(self._ff_seq)
        self._fold_wet_mask(tables=False)
        # The kernel also accumulates the tile counts of the transportmatrix these fluxes will be handed to (same mlotst, weighting, indices):
        # that call then has no counting pass.  (The library falls back to the plain kernel where it cannot count: nx < 3, OTMB_COUNT_IN_FF=0.)
        if not self.count_in_ff:
            self.ctx.check(self.lib.otmb_facefluxes_flags_dev(self.ctx.handle, umo.data_ptr(), vmo.data_ptr(),
                                                              int(umo.dtype == torch.float32), self.wetflags.data_ptr(), float(fill),
                                                              self.nx, self.ny, self.nz, self.topology, C.byref(ptrs), None,
                                                              self.push_mask.data_ptr()))
            self._mask_key = self._phi_key(self.phi)
            return self.phi
        cnt = capi.FfCounts()
        cnt.tables, cnt.lwet3d = self.count_tables.data_ptr(), self.lwet3d.data_ptr()
        cnt.mlotst, cnt.zt, cnt.n_wet = self.mlotst.data_ptr(), self.zt.data_ptr(), self.N
        cnt.upwind, cnt.only_t = int(self.upwind), 1 if self.only_T else 0
        self.ctx.check(self.lib.otmb_facefluxes_counts_dev(self.ctx.handle, umo.data_ptr(), vmo.data_ptr(),
                                                           int(umo.dtype == torch.float32), self.wetflags.data_ptr(), float(fill),
                                                           self.nx, self.ny, self.nz, self.topology, C.byref(ptrs),
                                                           self.push_mask.data_ptr(), C.byref(cnt)))
        self._mask_key = self._phi_key(self.phi)
        return self.phi

    def _note(self, calls):
        """Asynchronous calls of both kinds (calls: _ff_seq or _tm_seq) are numbered in one sequence, so that finish() can tell which of a
        facefluxes failure (counted among facefluxes calls) and a transportmatrix failure (counted among transportmatrix calls) came
        FIRST even when the two kinds of call were not issued in pairs."""
        self._seq += 1
        calls.append(self._seq)

    def _phi_key(self, phi):
        # the mask (and the tile counts that came with it) describes exactly the values facefluxes wrote, and the mixed-layer inputs and
        # weighting it was told: any later in-place torch op bumps _version
        return tuple((p.data_ptr(), p._version) for p in (*phi, self.mlotst, self.zt)) + (bool(self.upwind), bool(self.only_T))

    PIPELINE_DEPTH = 60  # the library remembers the verdicts of its 64 most recent asynchronous calls: drain before that

    def _first_missing(self):
        """Index (among the facefluxes calls since the previous check) of the first call whose umo or vmo held no valid
        value at all (the reference asserts per call, velocities.jl:199-200), or None; n = number of calls examined."""
        cap = 64
        u, v, n = (C.c_int32 * cap)(), (C.c_int32 * cap)(), C.c_int32(0)
        self.ctx.check(self.lib.otmb_facefluxes_pending_flags(self.ctx.handle, cap, u, v, C.byref(n)))
        self._ff_pending = 0
        self._ff_seq_drained, self._ff_seq = self._ff_seq[-n.value:] if n.value else [], []
        for q in range(n.value):
            if not (u[q] and v[q]):
                return q, n.value
        return None, n.value

    def _check_missing(self):
        bad, n = self._first_missing()
        if bad is not None:
            where = f" (asynchronous step {bad + 1} of {n})" if n > 1 else ""
            raise capi.OtmbError(8, self.lib.otmb_status_string(8).decode() + where, step=bad)

    def finish_facefluxes(self):
        """Drain a pipeline of facefluxes_async calls (no transportmatrix): raises the assertion of the first field
        without any valid value."""
        self._check_missing()
        return self.phi

    def step_async(self, umo, vmo, fill):
        """Enqueue one pass of the hot path (facefluxes -> count -> scan -> fill) without any host synchronisation;
        successive calls pipeline on the stream.  finish() synchronises and raises what the FIRST failing pass found
        (every pass keeps its own error flags on the device; OtmbError.step is its index)."""
        self._make_room()
        out = self.transportmatrix_onepass(self.facefluxes_async(umo, vmo, fill), sync=False)
        self._ff_pending += 1
        return out

    def _make_room(self):  # (drain before a step that would make the pipeline deeper than the library's memory of verdicts)
        if self._ff_pending >= self.PIPELINE_DEPTH:
            self.finish()

    def step_fused_async(self, umo, vmo, fill, out=None):
        """Extension (otmb_step_dev): one pass from (umo, vmo) to the five matrices WITHOUT the six ϕ arrays in memory -- only ϕtop is stored,
        the fill pass re-derives the other five fluxes from umo / vmo where it uses them.  The same matrices bit for bit as step_async, 64
        bytes per cell less HBM traffic.  Not the drop-in path: facefluxesfrommasstransport returns the six arrays."""
        self._make_room()
        if self.phi_top is None:
            self.phi_top = self._empty(self.G, torch.float64)
        out = self._output_set(out)
        self._fold_wet_mask(tables=True)
        self._mask_key = None
        a = self._args([self.phi_top] * 6)
        a.kept_ops, kept = self._kept_ops(out)
        cp, rv, nz = self._out_ptrs(out)
        caps = (C.c_int64 * 5)(*self._capacities())
        self._note(self._ff_seq)
        self._check(self.lib.otmb_step_dev(self.ctx.handle, umo.data_ptr(), vmo.data_ptr(), int(umo.dtype == torch.float32), float(fill),
                                           self.wetflags.data_ptr(), self.count_tables.data_ptr(), self.phi_top.data_ptr(), C.byref(a),
                                           C.byref(cp), C.byref(rv), C.byref(nz), C.byref(caps)))
        self._kept_written(out, kept)
        self._note(self._tm_seq)
        self._ff_pending += 1
        return out

    def finish(self):
        """Drain the pipeline: the earliest failing step wins; within a step facefluxes' assertion comes first, as in
        the reference (facefluxes runs before transportmatrix)."""
        bad, n = self._first_missing()
        ff_seq = self._ff_seq_drained
        tm_seq, self._tm_seq = self._tm_seq, []
        err = None
        try:
            out = self.result()
        except capi.OtmbError as e:
            err = e
        ff_first = True
        if bad is not None and err is not None and err.step is not None and bad < len(ff_seq) and err.step < len(tm_seq):
            ff_first = ff_seq[bad] < tm_seq[err.step]  # which of the two calls was issued first
        if bad is not None or err is not None:
            self._forget_kept()
        if bad is not None and (err is None or err.step is None or ff_first):
            where = f" (asynchronous step {bad + 1} of {n})" if n > 1 else ""
            raise capi.OtmbError(8, self.lib.otmb_status_string(8).decode() + where, step=bad)
        if err is not None:
            raise err
        return out

    def _args(self, phi):
        a = capi.TmArgs()
        a.nx, a.ny, a.nz = self.nx, self.ny, self.nz
        a.topology, a.upwind, a.n_wet = self.topology, int(self.upwind), self.N
        for k in range(6):
            a.phi[k] = phi[k].data_ptr()
        a.v3d, a.thkcello = self.v3d.data_ptr(), self.thk.data_ptr()
        a.rho = self.rho.data_ptr() if self.rho is not None else None
        a.rho_scalar = self.rho_scalar
        a.lwet3d = self.lwet3d.data_ptr()
        a.lwet = self.lwet.data_ptr()
        for k in range(4):
            a.edge_length[k] = self.edge[k].data_ptr()
            a.dist_nbr[k] = self.dist[k].data_ptr()
        a.area2d, a.zt, a.mlotst = self.area.data_ptr(), self.zt.data_ptr(), self.mlotst.data_ptr()
        a.kappa_h, a.kappa_vml, a.kappa_vdeep = self.kappa
        # ϕ straight from this object's facefluxes and untouched since: hand over its push mask
        fresh = self._mask_key is not None and self._mask_key == self._phi_key(phi)
        a.push_mask = self.push_mask.data_ptr() if fresh else None
        a.only_t = 1 if self.only_T else 0  # extension: materialise T alone (outputs of the operators unused)
        if self.given:
            for m, name in enumerate(MATS):
                if name in self.given:
                    cp, rv, nz = self.given[name]
                    a.given[m].colptr, a.given[m].rowval, a.given[m].nzval, a.given[m].nnz = cp.data_ptr(), rv.data_ptr(), nz.data_ptr(), rv.numel()
            key = self._given_versions()  # the library keys its verdicts to addresses: any in-place edit (torch bumps _version) makes it look again
            if key != self._given_key:
                self.ctx.forget_given()
                self._given_key = key
        return a

    def _out_ptrs(self, out):
        """The three pointer arrays of an output set; NULL for an operator the caller passes (nothing of it is written)."""
        skip = set(self.given)
        return tuple(capi.ptr_array(5, [None if m in skip else out[m][q].data_ptr() for m in MATS]) for q in range(3))

    # ---- kept operators (otmb_tm_args.kept_ops) ---------------------------------------------------------------------------------------------
    # TκH, TκVML and TκVdeep depend on the grid, κ and mlotst alone.  An output set whose three operators the library wrote in an earlier
    # successful call, untouched by torch since (the _version of its nine tensors is what it was then), is handed back with the promise: the fill
    # pass then stores T and Tadv only.  The library checks the promise against its own record and writes in full where it does not hold.
    KEPT = ("TκH", "TκVML", "TκVdeep")

    def _forget_kept(self):
        """The next call writes all five matrices (grid, κ, given operators changed; outputs overwritten; an error)."""
        self._kept = self._tpat = self._rho_kept = None
        self._kept_last, self._tpat_last = (), False
        for rec in self._ops.values():  # (and no operator's pattern can be vouched for any more)
            rec.ok = False

    def _kept_inputs(self, out):
        # the output set's nine tensors (by identity: a recycled address is another set), every grid array the three operators are derived from, κ
        same = [t for m in self.KEPT for t in out[m]]
        grid = [self.lwet3d, self.lwet, self.v3d, self.thk, self.area, self.zt, self.mlotst, *self.edge, *self.dist]
        return same, grid, self.kappa

    # T's pattern (OTMB_KEPT_T_PATTERN) is a function of the wet mask and the topology alone: when T's colptr / rowval tensors are the ones the
    # library last wrote, untouched by torch since, a step that keeps the three operators adds the bit and the fill stores T's values only (the
    # library checks its own record as well).  Tracked apart from _kept / _kept_last: the snapshot _tpat of out["T"][:2].
    # ρ is no grid constant and none of the kept operators' keys, so the library cannot know that it is unchanged: OTMB_KEPT_RHO says that the
    # ρ tensor is the one, at the version, of the last accepted call (by identity: a recycled address is another tensor).  The kept fill then
    # takes v3D and ρ from a table it builds once; a loop whose ρ changes every step never makes the promise and never builds it.
    def _kept_ops(self, out):
        """kept_ops for a call into `out`, and the names it covers."""
        self._kept_last, self._tpat_last = (), False
        self._tpat_fills0 = self.ctx.kept_t_pattern_fills()  # (what the library did with the promise: _ops_written compares)
        if self._kept is None or self.given or self.only_T or not self._kept.matches(*self._kept_inputs(out)):
            return 0, ()
        self._tpat_last = self._tpat is not None and self._tpat.matches(out["T"][:2])
        rho = self._rho_kept is not None and self.rho is not None and self._rho_kept.matches((self.rho,))
        return (sum(1 << MATS.index(m) for m in self.KEPT) | (capi.KEPT_T_PATTERN if self._tpat_last else 0)
                | (capi.KEPT_RHO if rho else 0)), self.KEPT

    def _kept_written(self, out, kept):
        """After a call into `out` was accepted: it wrote (or kept) the three operators unless some were given / not wanted."""
        self._kept_last = kept
        off = self.given or self.only_T or not self._kept_on
        self._kept = None if off else _Snapshot(*self._kept_inputs(out))
        self._tpat = None if off else _Snapshot(out["T"][:2])  # (T's pattern: written by this call, or where the last one left it)
        self._rho_kept = None if off or self.rho is None else _Snapshot((self.rho,))  # (ρ as this call read it: OTMB_KEPT_RHO)
        self._ops_written(out, kept)

    # ---- resident operators (otmb_op_*): one per output matrix, re-planned unless its pattern is shown unchanged ----------------------------
    def _ops_written(self, out, kept):
        """A call into `out` was accepted: the values of its matrices changed; an operator over one of them keeps its plan only if this call
        left the pattern where it was -- T: stored its values only (the KEPT_T_PATTERN promise made, and THIS fill took it: the library's count
        of values-only fills, otmb_ctx_kept_t_pattern_fills, went up by one since the call's _kept_ops -- otmb_ctx_kept_t_pattern alone would
        still hold an older fill's answer when the library declined the kept operators); TκH / TκVML / TκVdeep: kept; Tadv never.  (An exact
        cancellation compacts T when the step is folded: operator() compares nnz as well.)"""
        self._op_last_out = out
        if not self._ops:
            return
        f0 = self._tpat_fills0
        tpat = bool(self._tpat_last) and f0 is not None and self.ctx.kept_t_pattern_fills() == f0 + 1
        for name, rec in self._ops.items():
            if not (rec.snapshot.same_objects(out[name][:2]) and rec.nzv.same_objects(out[name][2:])):
                continue  # another output set: untouched
            rec.dirty = True
            if name == "T":
                rec.ok = rec.ok and tpat
            else:
                rec.ok = rec.ok and name in kept

    def _op_record(self, matrix):
        """What operator() and keep_slot() decide on: (the record of the operator over `matrix` or None, whether its plan holds for the result
        as it stands, the result's three tensors).  Pending asynchronous steps are folded first (finish()).  A record whose
        pattern cannot be vouched for but whose operator carries kept slots is compared with the copy of the pattern keep_slot took."""
        if self._tm_seq:
            self.finish()
        if self.out is None:
            raise ValueError("no resident result: run a step first")
        k = MATS.index(matrix)
        cp, rv, nz = self.out[matrix]
        rec = self._ops.get(matrix)
        nnz_now = self.nnz[k] if self._op_last_out is self.out else None
        live = rec is not None and bool(rec.op.handle.value) and nnz_now is not None and rec.op.nnz == nnz_now
        holds = live and rec.ok and rec.nzv.same_objects((nz,)) and rec.snapshot.matches((cp, rv))
        if live and not holds and rec.pattern is not None:
            self.ctx.synchronize()
            if torch.equal(cp, rec.pattern[0]) and torch.equal(rv[:nnz_now], rec.pattern[1]):
                # (dirty: whatever nzv says, the values are read again before the operator is handed out)
                rec.ok, rec.dirty, rec.snapshot, rec.nzv = True, True, _Snapshot((cp, rv)), _Snapshot((nz,))
                holds = True
        return rec, holds, (cp, rv, nz)

    def _slotted(self, matrix):
        """The record of the live operator over `matrix`, for the calls that work on its kept slots."""
        rec = self._ops.get(matrix)
        if rec is None or not rec.op.handle.value:
            raise ValueError(f"no operator over {matrix}: keep_slot() first")
        return rec

    @staticmethod
    def _has_slots(rec):
        return rec is not None and bool(rec.op.handle.value) and rec.op.slots[0] > 1

    def operator(self, matrix="T"):
        """The resident operator over the result `matrix` of this assembler's output set (otmb_op_create_dev), for mul() on device
        tensors.  Planned again unless every call since the plan left the pattern in place (see _ops_written) and nnz, the tensors and
        their torch versions are those of the plan; otherwise, when only values can have changed, otmb_op_set_values_dev.  Pending
        asynchronous steps are folded first (finish()).  The assembler owns the operator: it is replaced, not updated, by a re-plan.
        An operator with more than one slot is neither refreshed nor replaced here (either would overwrite or drop kept values): when the
        result is newer than the selected slot this raises, and keep_slot() or forget_slots() says where the result goes."""
        rec, holds, (cp, rv, nz) = self._op_record(matrix)
        if holds:
            if rec.dirty or not rec.nzv.matches((nz,)):
                if self._has_slots(rec):
                    raise ValueError(f"the operator over {matrix} holds {rec.op.slots[0]} slots and the result has changed since one was "
                                     "written: keep_slot(slot) puts it into one, forget_slots() drops them")
                rec.op.set_values_dev(nz)
                rec.dirty, rec.nzv = False, _Snapshot((nz,))
            self.op_reuses += 1
            return rec.op
        if self._has_slots(rec):
            raise ValueError(f"the pattern of {matrix} changed (or cannot be shown unchanged) under an operator that holds "
                             f"{rec.op.slots[0]} slots: forget_slots() drops them, then the operator is planned again")
        if rec is not None:
            rec.op.close()
        op = Operator(self.ctx, self.N, self.N, cp, rv, nz)
        op.set_lines(self.vertical_lines())
        self._ops[matrix] = OpRecord(op, snapshot=_Snapshot((cp, rv)), nzv=_Snapshot((nz,)))
        self.op_replans += 1
        return op

    def submatrix(self, rows, cols=None, matrix="T"):
        """Operator.submatrix of the resident operator over `matrix`: the kept slots' operator as it stands where slots are kept, operator()
        otherwise.  rows, cols: boolean masks or ascending 0-based index tensors on this GPU; cols=None: the principal submatrix, which has
        the grid's water columns restricted as its lines.  The CALLER owns the result (close it, or let it go): the assembler keeps no record
        of it, never refreshes or replaces it, and its own operator and slots are as they were; child.take_values(asm.operator(matrix))
        refreshes it after the next step while the assembler's operator is the same one."""
        rec = self._ops.get(matrix)
        op = rec.op if self._has_slots(rec) else self.operator(matrix)
        return op.submatrix(rows, cols)

    def vertical_lines(self):
        """The water columns of this grid as the `next` tensor of Operator.set_lines (api.vertical_lines on the resident indices, with torch
        ops): the wet rank of the cell below, where both are wet, else 0."""
        lw = self.lwet3d.view(self.nz, self.nx * self.ny)  # (level, horizontal cell) of Julia's column-major (nx, ny, nz)
        up, dn = lw[:-1].reshape(-1), lw[1:].reshape(-1)
        both = (up > 0) & (dn > 0)
        nxt = torch.zeros(self.N, dtype=torch.int64, device=self.device)
        nxt[up[both] - 1] = dn[both]
        return nxt

    def mul(self, matrix, X, *, alpha=1.0, beta=0.0, Y=None, adjoint=False):
        """Y = α·M·X + β·Y (adjoint: α·Mᵀ·X + β·Y) with M the resident result `matrix`, on torch device tensors (1-D, or rows x k
        column-major), bit for bit SparseArrays' mul!; no host round trip (besides folding pending asynchronous steps)."""
        return self.operator(matrix).mul(X, alpha=alpha, beta=beta, Y=Y, adjoint=adjoint)

    def solve(self, matrix, B, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False, precond="jacobi"):
        """X with (σ·I + diag(d) + M)·X = B (adjoint: ... + Mᵀ), M the resident result `matrix`, on torch device tensors: BiCGStab on the
        resident operator (Operator.solve), preconditioned by Jacobi or, precond="lines", by the grid's water columns (operator() sets them).
        Returns (X, info)."""
        return self.operator(matrix).solve(B, d=d, sigma=sigma, rtol=rtol, maxiter=maxiter, x0=x0, adjoint=adjoint, precond=precond)

    def keep_slot(self, slot, nslots=None, matrix="T"):
        """The resident result `matrix` as it stands becomes slot `slot` of its operator (the scatter from the device tensor, no host round
        trip) and that slot is selected, so mul() and solve() go on reading the result as it stands; nslots: grow the operator to that many
        slots first.  No other slot is written.  Built month by month, this is the year a tracer run cycles through.  The slots live on the
        operator and share its pattern: where the library did not vouch for the pattern, it is compared with a copy taken at the first
        keep_slot, and a result with another pattern raises (operator()) and leaves the slots as they are."""
        rec, holds, (cp, rv, nz) = self._op_record(matrix)
        if not holds:
            self.operator(matrix)  # no operator yet: planned over this result (one with slots and another pattern: raises)
            rec = self._ops[matrix]
        op = rec.op
        n, selected = op.slots
        if not 0 <= int(slot) < max(n, nslots or 0):
            raise ValueError(f"slot {slot} of {max(n, nslots or 0)}")
        if nslots is not None and nslots > n:
            op.set_slots(nslots)
        if int(slot) != selected or rec.dirty or not rec.nzv.matches((nz,)):
            op.set_values_dev(nz, slot=slot)
        op.select(slot)
        rec.dirty, rec.nzv = False, _Snapshot((nz,))
        if rec.pattern is None:
            self.ctx.synchronize()
            rec.pattern = (cp.clone(), rv[: op.nnz].clone())
        return op

    def forget_slots(self, matrix="T"):
        """Drop the operator over `matrix` with its slots; the next operator() / keep_slot() plans one over the result as it stands."""
        rec = self._ops.pop(matrix, None)
        if rec is not None:
            rec.op.close()

    def step_tracers(self, X, *, matrix="T", **kw):
        """Operator.step on the resident operator over `matrix` (named apart from step(), which builds a matrix): θ-steps of the tracers X
        through the slots keep_slot() filled, as they are -- a result built since and not kept takes no part; precond="lines" uses the
        grid's water columns."""
        return self._slotted(matrix).op.step(X, **kw)

    def step_tracers_sched(self, X, *, matrix="T", **kw):
        """Operator.step_sched on the resident operator over `matrix`: step_tracers with sub-steps per slot (substeps), a source per kept slot
        (a list of tensors) and a history (source_scale)."""
        return self._slotted(matrix).op.step_sched(X, **kw)

    def step_tracers_interp(self, X, *, matrix="T", **kw):
        """Operator.step_interp on the resident operator over `matrix`: step_tracers with the kept slots' matrices interpolated between slots
        (slot_a, slot_b, weight: api.interp_schedule makes them for monthly means valid at mid-month)."""
        return self._slotted(matrix).op.step_interp(X, **kw)

    def periodic_tracers_interp(self, source, *, matrix="T", **kw):
        """Operator.periodic_interp on the resident operator over `matrix`: periodic_tracers over a cycle of interpolated steps."""
        return self._slotted(matrix).op.periodic_interp(source, **kw)

    def step_tracers_season(self, X, *, matrix="T", **kw):
        """Operator.step_season on the resident operator over `matrix`: step_tracers_interp with d and the source per slot as well (lists of
        one or nslots tensors), blended with the matrices."""
        return self._slotted(matrix).op.step_season(X, **kw)

    def periodic_tracers_season(self, source, *, matrix="T", **kw):
        """Operator.periodic_season on the resident operator over `matrix`: the periodic state under a seasonal d and a seasonal source."""
        return self._slotted(matrix).op.periodic_season(source, **kw)

    def combine_slots(self, weights, dst, matrix="T"):
        """Operator.combine_slots on the resident operator over `matrix`: slot dst = Σ_s weights[s]·(slot s) over the slots keep_slot() filled
        (the annual mean of the kept months).  The written slot is not the resident result: when it is the selected one, the operator counts
        as changed since the result was put there, so operator() raises until keep_slot() or forget_slots() says where the result goes."""
        rec = self._slotted(matrix)
        rec.op.combine_slots(weights, dst)
        if int(dst) == rec.op.slots[1]:
            rec.dirty = True
        return rec.op

    def sinking(self, w, seafloor="open"):
        """The settling operator S of particles that sink at the speed w >= 0 (m/s, positive downward) on the resident grid
        (otmb_build_sink_dev; api.buildTsink states the contract): device tensors (colptr, rowval, nzval), no host round trip but the call's
        own checks.  w: a number, nz values (the bottom face of each level) or nx·ny·nz values (the bottom face of each cell, in the grid's
        column-major order; a (nx, ny, nz) array or tensor is taken in that order); a float64 tensor on this GPU is read where it lies, anything
        else is uploaded.  seafloor: "open" (default) or "closed".  asm.add_matrix(asm.sinking(w)) adds S to the kept slots."""
        closed = capi.seafloor_code(seafloor)
        form, ws, wt = 0, 0.0, None
        if torch.is_tensor(w) and w.dim() > 0:
            _on_device(w, self.device.index, "w")
            if w.dtype != torch.float64:
                raise ValueError("w: a float64 tensor is required")
            if w.dim() not in (1, 3) or (w.dim() == 3 and tuple(w.shape) != self.shape):
                raise capi.OtmbError(11, f"DimensionMismatch: w of {tuple(w.shape)}, expected a number, {(self.nz,)}, {(self.G,)} or {self.shape}")
            wt = (w.permute(2, 1, 0) if w.dim() == 3 else w).contiguous().view(-1)
        elif np.ndim(w) > 0:
            a = np.asarray(w, dtype=np.float64)
            if a.ndim not in (1, 3) or (a.ndim == 3 and a.shape != self.shape):
                raise capi.OtmbError(11, f"DimensionMismatch: w of {a.shape}, expected a number, {(self.nz,)} or {self.shape}")
            wt = self._t(a)
        else:
            ws = float(w)
        if wt is not None:
            if wt.numel() not in (self.nz, self.G):
                raise capi.OtmbError(11, f"DimensionMismatch: w of {wt.numel()} values, expected a number, {self.nz} or {self.G}")
            form = 1 if wt.numel() == self.nz else 2  # (nz == nx·ny·nz is a grid of one column: the two forms are one)
        cap = max(2 * self.N, 1)
        cp, rv, nz = self._empty(self.N + 1, torch.int64), self._empty(cap, torch.int64), self._empty(cap, torch.float64)
        nnz = C.c_int64(0)
        self.ctx.check(self.lib.otmb_build_sink_dev(self.ctx.handle, form, ws, None if wt is None else wt.data_ptr(), self.v3d.data_ptr(),
                                                    self.area.data_ptr(), self.lwet3d.data_ptr(), self.lwet.data_ptr(), self.N, self.nx, self.ny,
                                                    self.nz, closed, cp.data_ptr(), rv.data_ptr(), nz.data_ptr(), cap, C.byref(nnz)))
        k = int(nnz.value)
        return cp, rv[:k], nz[:k]

    def add_matrix(self, B, alpha=1.0, slots=None, matrix="T"):
        """Operator.add_matrix on the resident operator over `matrix`: slot = slot + alpha·B in place over the slots keep_slot() filled (slots:
        None = every slot, an int, or a list), for B = (colptr, rowval, nzval) device tensors whose pattern lies inside the matrix's --
        sinking()'s S, or one of this assembler's own results (a diffusivity retuned: B = out["TκH"], alpha = κ'/κ - 1).  Like
        combine_slots, a write to the selected slot makes the operator count as changed since the result was put there: operator() raises
        until keep_slot() or forget_slots() says where the result goes."""
        rec = self._slotted(matrix)
        rec.op.add_matrix(B, alpha=alpha, slots=slots)
        n, selected = rec.op.slots
        written = range(n) if slots is None else [int(x) for x in np.atleast_1d(np.asarray(slots))]
        if float(alpha) != 0.0 and B[1].numel() > 0 and selected in written:
            rec.dirty = True
        return rec.op

    def periodic_tracers(self, source, *, matrix="T", **kw):
        """Operator.periodic on the resident operator over `matrix`: the periodic state of the cycle through the slots keep_slot() filled, as
        they are (step_tracers says which slots those are); outer="mean" preconditions the outer iteration with their cycle mean."""
        return self._slotted(matrix).op.periodic(source, **kw)

    def periodic_tracers_sched(self, source, *, matrix="T", **kw):
        """Operator.periodic_sched on the resident operator over `matrix`: periodic_tracers with sub-steps per slot and a source per kept slot."""
        return self._slotted(matrix).op.periodic_sched(source, **kw)

    def _kept_steady(self):
        """The operators a step of this loop does not store: those the last call kept, or -- after a full write that left the promise live -- those
        the next call will keep (what every launch after the first one of a time loop writes: bench.py's roofline reads this after its extras)."""
        return set(self._kept_last) | (set(self.KEPT) if self._kept is not None else set())

    def _htab_bytes(self, skip):
        """Bytes of the library's TκH table that a fill pass which keeps all three operators (`skip`) reads: five Float64 per wet column.  Such
        a pass does not read thkcello and the eight edge / distance arrays (the tripolar seam row aside: one row of cells).  Whether the table
        is read is the library's answer for the last such fill (otmb_ctx_kept_htab; before the first one: the library's own rule -- nx >= 3
        and OTMB_KEPT_HTAB as this process started).  0: TκH is re-derived from thkcello and the metrics."""
        if not set(self.KEPT) <= skip or self.given:
            return 0
        used = self.ctx.kept_htab()
        return 40 * self.N if (used == 1 or (used < 0 and self.nx >= 3 and _KEPT_HTAB_ON)) else 0

    def _tpat_steady(self, skip):
        """Whether a kept step of this loop (`skip`) stores T's values only: its colptr and rowval are then not written.  Like _kept_steady, the
        time loop's steady state: the promise was made or is live for the next call, the TκH table is read (the library takes the pattern on
        that path only) and OTMB_KEPT_TPAT was not 0 as this process started.  (Whether the last fill took it, otmb_ctx_kept_t_pattern, also
        depends on whether the record's writer has been folded yet: the first steps of a pipeline write T in full.)"""
        if not set(self.KEPT) <= skip or self.given or "T" in skip:
            return False
        if not (self._tpat_last or self._tpat is not None):
            return False
        return _KEPT_TPAT_ON and self._htab_bytes(skip) > 0

    def _check(self, rc):
        try:
            self.ctx.check(rc)
        except capi.OtmbError:
            self._forget_kept()
            raise

    def plan(self, phi):
        a = self._args(phi)
        kept = ()
        if self.out is not None:
            a.kept_ops, kept = self._kept_ops(self.out)
        nnz = (C.c_int64 * 5)()
        self._check(self.lib.otmb_transportmatrix_plan_dev(self.ctx.handle, C.byref(a), C.byref(nnz)))
        self.nnz = [int(x) for x in nnz]
        self._plan_kept = (phi, kept)
        return self.nnz

    def fill(self):
        """Write the five CSC matrices into device tensors (allocated once per capacity)."""
        if self.out is None or any(self.out[m][1].numel() < self.nnz[k] for k, m in enumerate(MATS)):
            phi, kept = self._plan_kept
            self._forget_kept()
            if kept:  # (the plan counted on the old arrays of the kept operators: plan again without the promise, then allocate)
                self.plan(phi)
            self._out_cap = None
            self.out = {m: self._csc(self.N, max(z, 1) + z // 64) for m, z in zip(MATS, self.nnz)}
        cp, rv, nz = self._out_ptrs(self.out)
        kept = self._plan_kept[1]
        self._plan_kept = (None, ())
        self._check(self.lib.otmb_transportmatrix_fill_dev(self.ctx.handle, C.byref(cp), C.byref(rv), C.byref(nz)))
        self._kept_written(self.out, kept)
        final = (C.c_int64 * 5)()
        self.ctx.check(self.lib.otmb_transportmatrix_nnz(self.ctx.handle, C.byref(final)))
        self.nnz = [int(x) for x in final]  # T's planned count is an upper bound
        return self.out

    def transportmatrix(self, phi):
        """Two-phase protocol (what a caller that must size its outputs first does): plan, then fill."""
        self.plan(phi)
        return self.fill()

    PER_COLUMN_MAX = (7, 7, 5, 3, 3)  # rows a column of T, Tadv, TκH, TκVML, TκVdeep can hold
    FILL_KERNELS = ("tm_kernel<fill>",)  # the pass that writes the matrices (otmb_kernel_name)

    def new_output_set(self):
        """A set of five CSC output buffers at their upper bound (for transportmatrix_onepass(out=...): a pipeline whose
        steps each keep their own matrices)."""
        return {m: self._csc(self.N, cap) for m, cap in zip(MATS, self._capacities())}

    def _csc(self, cols, cap):
        """(colptr, rowval, nzval) device arrays of a matrix of `cols` columns with room for `cap` entries."""
        return self._empty(cols + 1, torch.int64), self._empty(cap, torch.int64), self._empty(cap, torch.float64)

    def _capacities(self):
        """Entries the five matrices can hold at most, + 1 (the lengths of new_output_set()'s rowval / nzval arrays)."""
        return [self.N * k + 1 for k in self.PER_COLUMN_MAX]

    def _output_set(self, out):
        """The output set an asynchronous call writes: `out`, or this object's own at the capacities -- made at the first call, and again
        where fill() left one sized to its plan."""
        if out is not None:
            return out
        if self.out is None or self._out_cap is None:
            self.out = self.new_output_set()
            self._out_cap = self._capacities()
        return self.out

    def choose_placement(self, umo, vmo, fill, candidates=4, reps=3, budget_fraction=0.6, min_output_bytes=4 << 30):
        """Set-up time only, never results: pick WHERE this assembler's flux arrays and output matrices live.
        On MI355X the time of the two write-heavy passes depends reproducibly on which device allocations their arrays were given -- inside one
        process the fill pass ran 5.86 ... 6.57 ms (another box: 5.97 ... 7.35 ms) on eight output sets whose virtual layout is identical, every set
        repeating to 0.1 % (profiles/r04/README.md section 12): it is the physical backing of the ~30 concurrently streamed arrays that differs, and
        no per-buffer probe sees it (single streams differ by <= 4 %).  So: allocate `candidates` flux sets and time facefluxes on each, keep the fastest;
        then `candidates` output sets (new_output_set()) and time the fill pass on each with the kept fluxes, keep the fastest; free the rest.
        Nothing is chosen when the candidates would not fit in `budget_fraction` of the free device memory (the 0.1 degree grid), nor on grids whose
        output set is smaller than `min_output_bytes` (1 degree: the candidates differ by 1-2 % there, nothing to choose).  Returns a record of every
        candidate's time (bench.py prints it)."""
        rec = {"candidates": int(candidates), "facefluxes_ms": [], "fill_ms": [], "chosen": None}
        self._forget_kept()  # (every candidate output set is written in full: what is timed is the full fill pass)
        if candidates < 2:
            return rec
        free_b, _ = torch.cuda.mem_get_info(self.device)
        phi_bytes = self.G * (6 * 8 + 2)
        out_bytes = sum(cap * 16 + (self.N + 1) * 8 for cap in self._capacities())
        if out_bytes < min_output_bytes:
            rec["skipped"] = "small grid: placements differ by 1-2 %"
            return rec
        if candidates * (phi_bytes + out_bytes) > budget_fraction * free_b:
            rec["skipped"] = "candidates do not fit"
            return rec

        def timed(kernels, launch):
            """mean duration of the pass `kernels` names"""
            for _ in range(2):
                launch()
            self.ctx.synchronize()
            self.ctx.timing_enable(True)
            for _ in range(reps):
                launch()
            self.ctx.synchronize()
            t = self.ctx.timing_collect()
            self.ctx.timing_enable(False)
            ran = [t[k] for k in kernels if k in t]
            if not ran:
                raise RuntimeError(f"choose_placement: none of {kernels} was launched ({sorted(t)})")
            return max(ms / cnt for ms, cnt in ran)

        phis = [([self._empty(self.G, torch.float64) for _ in range(6)], self._empty(self.G, torch.int16)) for _ in range(candidates)]
        for p, m in phis:
            self.phi, self.push_mask = p, m
            rec["facefluxes_ms"].append(timed(("facefluxes_kernel",), lambda: self.facefluxes_async(umo, vmo, fill)))
        self.finish_facefluxes()
        kp = int(np.argmin(rec["facefluxes_ms"]))
        self.phi, self.push_mask = phis[kp]
        del phis, p, m
        phi = self.facefluxes(umo, vmo, fill)
        outs = [self.new_output_set() for _ in range(candidates)]
        for o in outs:
            self._forget_kept()
            rec["fill_ms"].append(timed(self.FILL_KERNELS, lambda: (self._forget_kept(), self.transportmatrix_onepass(phi, sync=False, out=o))))
            self.result()
        self._forget_kept()
        ko = int(np.argmin(rec["fill_ms"]))
        self.out, self._out_cap = outs[ko], self._capacities()
        del outs, o
        torch.cuda.empty_cache()  # the candidates that were not kept go back to the driver
        rec["chosen"] = [kp, ko]
        return rec

    def transportmatrix_onepass(self, phi, sync=True, out=None):
        """Asynchronous protocol (otmb_transportmatrix_dev): outputs preallocated at their upper bound, count ->
        scan -> fill enqueued without a host round trip.  With sync=False the nnz/errors are collected later by
        result().  out: an output set of new_output_set() (default: this object's one set, overwritten by every call)."""
        out = self._output_set(out)
        a = self._args(phi)
        a.kept_ops, kept = self._kept_ops(out)
        cp, rv, nz = self._out_ptrs(out)
        caps = (C.c_int64 * 5)(*self._capacities())
        self._check(self.lib.otmb_transportmatrix_dev(self.ctx.handle, C.byref(a), C.byref(cp), C.byref(rv),
                                                      C.byref(nz), C.byref(caps)))
        self._kept_written(out, kept)
        self._note(self._tm_seq)
        return self.result() if sync else out

    def result(self):
        nnz = (C.c_int64 * 5)()
        rc = self.lib.otmb_transportmatrix_result(self.ctx.handle, C.byref(nnz))
        self._tm_seq = []
        if rc != capi.OK:
            self._forget_kept()
            step = C.c_int64(-1)
            self.lib.otmb_transportmatrix_failed_step(self.ctx.handle, C.byref(step))
            raise capi.OtmbError(rc, self.lib.otmb_last_error(self.ctx.handle).decode("utf-8"),
                                 step=int(step.value) if step.value >= 0 else None)
        self.nnz = [int(x) for x in nnz]
        return self.out

    def result_step(self, k):
        """(status, nnz) of the k-th asynchronous call covered by the last result(): every call keeps its own verdict and
        its own nnz (and its own T, compacted if entries cancelled, when it was given its own output arrays)."""
        nnz = (C.c_int64 * 5)()
        rc = self.lib.otmb_transportmatrix_result_step(self.ctx.handle, int(k), C.byref(nnz))
        return rc, [int(x) for x in nnz]

    def step(self, umo, vmo, fill, onepass=True):
        """One pass of the hot path, all device resident: facefluxes -> transportmatrix."""
        phi = self.facefluxes(umo, vmo, fill)
        return self.transportmatrix_onepass(phi) if onepass else self.transportmatrix(phi)

    def lump_and_spray(self, mask=None, di=2, dj=2, dk=1, matrix="T"):
        """lump_and_spray (src/extratools.jl:38-119) on the resident grid and the resident result `matrix` (only its
        pattern is read; the volumes are v3D on the wet cells).  mask: flat uint8/bool device tensor or None.
        Returns device tensors: LUMP (colptr, rowval, nzval), SPRAY (colptr, rowval, nzval), vol_c."""
        k = MATS.index(matrix)
        cp, rv, _ = self.out[matrix]
        m = None
        if mask is not None:
            m = mask.to(self.device).reshape(-1).to(torch.uint8).contiguous()
            if m.numel() != self.G:
                raise ValueError("mask must have one entry per grid cell")
        nc = C.c_int64(0)
        self.ctx.check(self.lib.otmb_lump_and_spray_plan_dev(
            self.ctx.handle, self.wet3d.data_ptr(), None if m is None else m.data_ptr(), self.lwet3d.data_ptr(),
            self.lwet.data_ptr(), self.N, self.nx, self.ny, self.nz, cp.data_ptr(), rv.data_ptr(), int(di), int(dj), int(dk),
            C.byref(nc)))
        Nc, N = int(nc.value), self.N
        vol = self.v3d[self.lwet[:N] - 1].contiguous()
        i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=self.device)
        f64 = lambda n: torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
        L = (i64(N + 1), i64(N), f64(N))
        S = (i64(Nc + 1), i64(N), f64(N))
        vc = f64(Nc)
        self.ctx.check(self.lib.otmb_lump_and_spray_fill_dev(self.ctx.handle, vol.data_ptr(), L[0].data_ptr(), L[1].data_ptr(),
                                                             L[2].data_ptr(), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                                             vc.data_ptr()))
        return (L[0], L[1][:N], L[2][:N]), (S[0], S[1][:N], S[2][:N]), vc[:Nc]

    def coarsen(self, L, S, matrix="T", m=None):
        """C = L * matrix * S (the coarse operator; src/extratools.jl:14-16) on the device, bit for bit SparseArrays' (L * T) * S.
        L, S: (colptr, rowval, nzval) device tensors as lump_and_spray returns them (L: Nc x N with at most one entry per column,
        S: N x n); `matrix` is the resident result.  m: the rows of L (default n, as for lump_and_spray's pair).  Only nnz travels
        to the host.  Returns (colptr, rowval, nzval) tensors."""
        cp, rv, nz = self.out[matrix]
        Lp, Li, Lx = (t.contiguous() for t in L)
        Sp, Si, Sx = (t.contiguous() for t in S)
        N = self.N
        if Lp.numel() != N + 1 or Sp.numel() < 1:
            raise ValueError("L must have N + 1 column pointers")
        n = Sp.numel() - 1
        m = n if m is None else int(m)
        nnz = C.c_int64(0)
        self.ctx.check(self.lib.otmb_coarsen_plan_dev(self.ctx.handle, m, N, Lp.data_ptr(), Li.data_ptr(), Lx.data_ptr(), N, cp.data_ptr(),
                                                      rv.data_ptr(), nz.data_ptr(), n, Sp.data_ptr(), Si.data_ptr(), Sx.data_ptr(),
                                                      C.byref(nnz)))
        k = int(nnz.value)
        Cp, Ci, Cx = self._csc(n, max(k, 1))
        self.ctx.check(self.lib.otmb_coarsen_fill_dev(self.ctx.handle, Cp.data_ptr(), Ci.data_ptr(), Cx.data_ptr()))
        return Cp, Ci[:k], Cx[:k]

    def result_to_host(self):
        self.ctx.synchronize()
        if any(self.out[m][1].numel() < self.nnz[k] for k, m in enumerate(MATS)):
            raise RuntimeError("output buffers smaller than nnz")
        res = {}
        for k, m in enumerate(MATS):
            cp, rv, nz = self.out[m]
            res[m] = (cp.cpu().numpy(), rv[: self.nnz[k]].cpu().numpy(), nz[: self.nnz[k]].cpu().numpy())
        return res

    # ---- the reference's two-step formulation (general path) ----------------------------------------------------
    def sparse_entries(self, which, phi=None):
        """COO triplets (I, J, V device tensors) of one operator in the reference's push order
        (advection/horizontal/vertical *_operator_sparse_entries, src/matrixbuilding.jl:221-479).
        which: "Tadv" | "TκH" | "TκVML" | "TκVdeep"."""
        code = {"Tadv": 0, "TκH": 1, "TκVML": 2, "TκVdeep": 3}[which]
        a = self._args(phi if phi is not None else self.phi)
        n = C.c_int64(0)
        self.ctx.check(self.lib.otmb_sparse_entries_plan_dev(self.ctx.handle, code, C.byref(a), C.byref(n)))
        ln = int(n.value)
        I = torch.empty(max(ln, 1), dtype=torch.int64, device=self.device)
        J = torch.empty(max(ln, 1), dtype=torch.int64, device=self.device)
        V = torch.empty(max(ln, 1), dtype=torch.float64, device=self.device)
        self.ctx.check(self.lib.otmb_sparse_entries_fill_dev(self.ctx.handle, I.data_ptr(), J.data_ptr(), V.data_ptr()))
        return I[:ln], J[:ln], V[:ln]

    def sparse(self, I, J, V, m, n):
        """SparseArrays.sparse(I, J, V, m, n) on the device -> (colptr, rowval, nzval) tensors."""
        I, J, V = I.contiguous(), J.contiguous(), V.contiguous()
        nnz = C.c_int64(0)
        self.ctx.check(self.lib.otmb_sparse_plan_dev(self.ctx.handle, I.data_ptr(), J.data_ptr(), V.data_ptr(), I.numel(), m, n,
                                                     C.byref(nnz)))
        k = int(nnz.value)
        cp, rv, nz = self._csc(n, max(k, 1))
        self.ctx.check(self.lib.otmb_sparse_fill_dev(self.ctx.handle, cp.data_ptr(), rv.data_ptr(), nz.data_ptr()))
        self.ctx.synchronize()
        return cp, rv[:k], nz[:k]

    def spadd(self, A, B, n):
        """A + B on the device (SparseArrays' map(+): union pattern, exact-zero sums dropped; src/matrixbuilding.jl:147).
        A, B: (colptr, rowval, nzval) device tensors of n columns; returns the same triple."""
        Ap, Ai, Ax = (t.contiguous() for t in A)
        Bp, Bi, Bx = (t.contiguous() for t in B)
        nnz = C.c_int64(0)
        self.ctx.check(self.lib.otmb_spadd_plan_dev(self.ctx.handle, n, Ap.data_ptr(), Ai.data_ptr(), Ax.data_ptr(), Bp.data_ptr(),
                                                    Bi.data_ptr(), Bx.data_ptr(), C.byref(nnz)))
        k = int(nnz.value)
        Cp, Ci, Cx = self._csc(n, max(k, 1))
        self.ctx.check(self.lib.otmb_spadd_fill_dev(self.ctx.handle, n, Ap.data_ptr(), Ai.data_ptr(), Ax.data_ptr(), Bp.data_ptr(),
                                                    Bi.data_ptr(), Bx.data_ptr(), Cp.data_ptr(), Ci.data_ptr(), Cx.data_ptr()))
        self.ctx.synchronize()
        return Cp, Ci[:k], Cx[:k]

    # ---- accounting ---------------------------------------------------------------------------
    def algorithmic_bytes(self):
        """bytes the assembly must move with all five matrices returned
        (inputs read once, outputs written once; intermediate traffic is overhead and not counted)."""
        r, w = self.algorithmic_bytes_split()
        return r + w

    def algorithmic_bytes_split(self):
        """(bytes read, bytes written) of algorithmic_bytes().  An operator the caller passes and the fill pass re-derives (set_given) is
        neither read nor written: its 16 nnz + 8 (N + 1) bytes are not part of the pass.  Nor is one the last call kept where the previous
        write left it, or that the next call keeps (otmb_tm_args.kept_ops: a time loop's steady state); when all three are kept the pass reads
        the library's TκH table instead of thkcello and the edge / distance metrics (_htab_bytes), and writes T's values only when its pattern
        is kept too (_tpat_steady: 8 nnz(T), no colptr, no rowval)."""
        skip = set(self.given) | self._kept_steady()
        htab = self._htab_bytes(skip)
        tpat = self._tpat_steady(skip)
        n3d = 9 + (1 if self.rho is not None else 0) - (1 if htab else 0)  # (thkcello)
        n2d = 10 - (8 if htab else 0)  # (the edge lengths and distances: area and mlotst stay)
        return (8 * self.G * n3d + 8 * n2d * self.nx * self.ny + 8 * self.nz + htab,
                sum((8 * z if (m == "T" and tpat) else 16 * z + 8 * (self.N + 1)) for m, z in zip(MATS, self.nnz) if m not in skip))

    def fill_pass_stream_mix(self):
        """What an ideal streaming kernel reaches over the fill pass's OWN arrays (otmb_ctx_stream_mix): its ten 3-D inputs (+ the 2-D
        metrics) read once, its fifteen output arrays written once at their actual lengths, in as many slices as the pass has tiles.
        DESTROYS the matrices of self.out: call it after the results have been used.  {columns per slice: GB/s}.  Operators the last call kept
        (otmb_tm_args.kept_ops) are not among the pass's outputs; when all three are kept, the pass's inputs are those of _htab_bytes: the TκH
        table (a stand-in with its layout, five arrays of N Float64: the library's own is not addressable from here) instead of thkcello and
        the edge / distance metrics."""
        b8 = lambda t, n=None: (t.data_ptr(), 8 * (t.numel() if n is None else n))
        skip = self._kept_steady()
        htab = self._htab_bytes(skip)
        tpat = self._tpat_steady(skip)
        self._forget_kept()
        ins = [b8(p) for p in self.phi] + [b8(self.v3d), b8(self.lwet3d)] + ([b8(self.rho)] if self.rho is not None else [])
        ins += [b8(t) for t in (self.area, self.mlotst)]
        if htab:
            slot = self.N + (self.N & 1)  # (16-byte aligned slots)
            stand_in = torch.empty(5 * slot, dtype=torch.float64, device=self.device)
            ins += [(stand_in[q * slot:].data_ptr(), 8 * self.N) for q in range(5)]
        else:
            ins += [b8(self.thk)] + [b8(t) for t in (*self.edge, *self.dist)]
        outs = []
        for k, m in enumerate(MATS):
            if m in skip:
                continue
            cp, rv, nz = self.out[m]
            outs += [b8(nz, self.nnz[k])] if (m == "T" and tpat) else [b8(cp, self.N + 1), b8(rv, self.nnz[k]), b8(nz, self.nnz[k])]
        # the fill pass's own granularity (256 columns per slice) and longer slices: a plain stream likes them longer where the grid is large
        # enough to still fill the chip (profiles/r05: 4.3 / 4.3 / 3.9 / 3.7 TB/s at 1 degree, 4.9 / 5.4 / 5.6 / 5.5 TB/s at 0.25 degree)
        return {cols: self.ctx.stream_mix(ins, outs, max(8, self.N // cols)) for cols in (256, 512, 1024, 2048)}

    def facefluxes_bytes(self, itemsize=8):
        """umo, vmo, wet3D read once; six ϕ arrays written once."""
        return self.G * (2 * itemsize + 1 + 6 * 8)
