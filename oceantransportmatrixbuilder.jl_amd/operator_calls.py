"""The resident operator's solver calls, marshalled once for both bindings: api.DeviceOperator (numpy arrays, the host-pointer exports) and
device.Operator (torch tensors, the `_dev` exports) derive from OperatorCalls, which validates the arguments, assembles each export's argument
list in the order of include/otmb.h and turns the status into a report.  The two classes differ only in how they handle arrays.  No torch
here: api.py imports without it."""
import ctypes as C

import numpy as np

from . import capi


class SolveInfo:
    """What otmb_op_solve_pc reports, one entry per column of B: iterations (completed), relres (‖r‖₂/‖b‖₂ of the column's last residual
    evaluation: the explicitly computed b - M·x when it stopped on one, the recursive residual otherwise), reason ("converged", "maxiter",
    "breakdown", "nonfinite") and converged; status is the call's own (0, or capi.NOT_CONVERGED when some column is not converged)."""

    def __init__(self, status, iterations, relres, reason):
        self.status = int(status)
        self.iterations = np.asarray(iterations, dtype=np.int64)
        self.relres = np.asarray(relres, dtype=np.float64)
        self.reason = tuple(capi.SOLVE_REASONS[int(r)] for r in reason)
        self.converged = np.array([r == "converged" for r in self.reason], dtype=bool)

    def __repr__(self):
        return f"SolveInfo(status={self.status}, iterations={self.iterations.tolist()}, relres={self.relres.tolist()}, reason={self.reason})"


class StepInfo:
    """What otmb_op_step reports: status (0, or capi.NOT_CONVERGED), steps_done (steps completed with every column converged) and, one row
    per step that ran a solve (steps 0 .. min(steps_done, nsteps - 1)) and one entry per column: iterations, relres, reason (tuples of
    "converged", "maxiter", "breakdown", "nonfinite") and converged -- each as SolveInfo has them for one solve.  From
    step(..., observe=W): observations, (steps_done, k, q), entry [t, c, j] = observer j of tracer c after step t (only the steps that were
    completed); from step(..., time_weights=w): mean, n x k (n values for a 1-D state) = Σ_t w[t]·X_t over the completed steps, None when
    no step was.  Both None otherwise."""

    def __init__(self, status, steps_done, nsteps, iterations, relres, reason, observations=None, mean=None):
        self.status, self.steps_done = int(status), int(steps_done)
        self.observations = None if observations is None else observations[:self.steps_done]
        self.mean = mean if self.steps_done > 0 else None
        ran = min(self.steps_done + 1, int(nsteps))
        self.iterations = np.asarray(iterations, dtype=np.int64)[:ran]
        self.relres = np.asarray(relres, dtype=np.float64)[:ran]
        self.reason = tuple(tuple(capi.SOLVE_REASONS[int(r)] for r in row) for row in np.asarray(reason)[:ran])
        self.converged = np.array([[r == "converged" for r in row] for row in self.reason], dtype=bool).reshape(self.iterations.shape)

    def __repr__(self):
        return f"StepInfo(status={self.status}, steps_done={self.steps_done}, iterations={self.iterations.tolist()}, reason={self.reason})"


def observers(W, n):
    """(W as a 2-D array n x q, q) of step(..., observe=W) / observe(W, X): n values are one observer."""
    shape = tuple(W.shape)
    if len(shape) not in (1, 2) or shape[0] != n:
        raise capi.OtmbError(11, f"DimensionMismatch: observers of {shape}, expected {n} rows")
    return (W.reshape(n, 1) if len(shape) == 1 else W), (1 if len(shape) == 1 else shape[1])


def time_weights(w, nsteps):
    """The mean's weights as nsteps float64 host values."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (max(int(nsteps), 0),):
        raise capi.OtmbError(11, f"DimensionMismatch: time_weights of {w.shape}, expected {(max(int(nsteps), 0),)}")
    return w


_as_weights = time_weights  # step has a keyword time_weights: inside it the function goes by this name


def step_arrays(nsteps, k):
    """The three report arrays of otmb_op_step (nsteps x k, step-major)."""
    shape = (max(int(nsteps), 0), int(k))
    return np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.float64), np.zeros(shape, dtype=np.int32)


class PeriodicInfo:
    """What otmb_op_periodic reports, one entry per column: cycles (the step calls the column took part in, the verifying ones included),
    defect (‖F(x) - x‖₂/‖g‖₂ of the column's last explicitly computed F(x) - x; NaN when none was), reason ("converged", "maxcycles",
    "step_failed", "nonfinite", and with outer="mean" "precond_failed") and converged; msolve_iters: the BiCGStab iterations the column spent in
    mean solves (outer="mean"; otherwise zero); status is the call's own (0, or capi.NOT_CONVERGED when some column is not converged)."""

    def __init__(self, status, cycles, defect, reason, msolve_iters=None):
        self.status = int(status)
        self.cycles = np.asarray(cycles, dtype=np.int64)
        self.defect = np.asarray(defect, dtype=np.float64)
        self.reason = tuple(capi.PERIODIC_PC_REASONS[int(r)] for r in reason)
        self.converged = np.array([r == "converged" for r in self.reason], dtype=bool)
        self.msolve_iters = np.zeros(len(self.cycles), dtype=np.int64) if msolve_iters is None else np.asarray(msolve_iters, dtype=np.int64)

    def __repr__(self):
        return (f"PeriodicInfo(status={self.status}, cycles={self.cycles.tolist()}, defect={self.defect.tolist()}, reason={self.reason}, "
                f"msolve_iters={self.msolve_iters.tolist()})")


class OperatorCalls:
    """add_matrix, precondition, solve, observe, step and periodic of a resident operator (its handle `_h`, `shape` and context `ctx`), written once.
    Arrays below are numpy arrays for api.DeviceOperator and float64 tensors on the operator's GPU for device.Operator, whose results --
    the states, info.observations and info.mean -- are new device tensors; the reports' per-column records and time_weights are host values
    for both.  What a subclass says about its arrays:
      _suffix               of the exports' names: "" (host pointers) or "_dev" (device pointers)
      _live()               raises ValueError when the operator is closed
      _library()            the loaded library
      _array(a, what)       the argument as an array of the class's kind (`what` names it in a refusal)
      _matrix(a, rows)      (a column-major, its leading dimension): `a` itself when its rows are contiguous, a copy otherwise
      _ptr(a)               the address the library is given (None stays None)
      _zeros(shape, order)  a zeroed float64 result: "F" column-major (rows x k with leading dimension max(rows, 1)), "C" row-major
      _assign(X, a)         copies a into the result X
    and, for the calls on the operator's domain (submatrix, take_values, to_csc, lines):
      _selection(s, limit, what)  a boolean mask of `limit` entries or an ascending 0-based index array as 1-based int64 indices of the class's kind
      _empty(n, dtype)      an uninitialised 1-D array of "int64" or "float64" for the library to fill
      _csc(cp, rv, nz)      what to_csc returns of the three filled arrays
      _adopt(h)             a new operator of the class over the handle h, on this operator's context
    and, for add_matrix:
      _csc_arrays(B)        (colptr, rowval, nzval) of a matrix of the operator's shape as int64, int64 and float64 arrays of the class's kind
    Every refusal is raised before the library is called, but for the order of a selection's indices, which the library checks on the device."""

    _suffix = ""

    def _call(self, name, *args):
        return getattr(self._library(), name + self._suffix)(self._h, *args)

    def _status(self, rc):
        """NOT_CONVERGED is an answer (the info object says which column stopped why); every other status but 0 raises."""
        if rc != capi.NOT_CONVERGED:
            self.ctx.check(rc)
        return rc

    def _state(self, B, what):
        """(B as an array, k, B column-major, its leading dimension) of the argument that has the state's shape: m values or m x k."""
        B = self._array(B, what)
        m, n = self.shape
        if B.ndim not in (1, 2) or B.shape[0] != m:
            raise capi.OtmbError(11, f"DimensionMismatch: operator of {(m, n)}, {what} of {tuple(B.shape)}")
        Bc, ldb = self._matrix(B, m)
        return B, (1 if B.ndim == 1 else B.shape[1]), Bc, ldb

    def _like(self, a, what, B, of):
        """x0 or source as an array: it has the shape of the state B (the argument `of`)."""
        a = self._array(a, what)
        if tuple(a.shape) != tuple(B.shape):
            raise capi.OtmbError(11, f"DimensionMismatch: {what} of {tuple(a.shape)}, {of} of {tuple(B.shape)}")
        return a

    def _check_d(self, d, want, what):
        """d has the shape `want`: (n,), or that of the state `what` for one d per column.  (device.Operator's also refuses other dtypes,
        which numpy converts, in the wording its tests know.)"""
        if tuple(d.shape) != want:
            raise capi.OtmbError(11, f"DimensionMismatch: d of {tuple(d.shape)}, " + (f"expected {want}" if len(want) == 1 else f"{what} of {want}"))

    def _d(self, d, B, what):
        """(what keeps d alive, d's part of an argument list): [pointer or None] for n values or None -- the exports with one d -- and
        [pointer, ldd] for a matrix of B's shape, one d per column: the otmb_op_*_dk exports (include/otmb.h: column c is the 1-D call with
        d[:, c], bit for bit)."""
        if d is None:
            return None, [None]
        d = self._array(d, "d")
        if d.ndim != 2:
            self._check_d(d, (self.shape[1],), what)
            dc, _ = self._matrix(d, self.shape[1])
            return dc, [self._ptr(dc)]
        if B.ndim != 2:
            raise capi.OtmbError(11, f"DimensionMismatch: d of {tuple(d.shape)} is per column, {what} of {tuple(B.shape)} has no columns")
        self._check_d(d, tuple(B.shape), what)
        Dc, ldd = self._matrix(d, self.shape[1])
        return Dc, [self._ptr(Dc), ldd]

    def _start(self, x0, B, of):
        """The zeroed result of B's shape, with x0 copied in when one is given."""
        if x0 is not None:
            x0 = self._like(x0, "x0", B, of)
        X = self._zeros(tuple(B.shape))
        if x0 is not None:
            self._assign(X, x0)
        return X

    def _sources(self, source, B, of):
        """(the blocks column-major, their common leading dimension) of a source given as a list or tuple of arrays of B's shape -- one for
        every step, or one per slot: the scheduled calls' array of pointers (include/otmb.h).  Blocks whose leading dimensions differ are
        copied compactly; nothing is stacked."""
        nslots = self.slots[0]
        if len(source) not in (1, nslots):
            raise capi.OtmbError(11, f"DimensionMismatch: {len(source)} source blocks, expected 1 or one per slot ({nslots})")
        m = self.shape[0]
        blocks = [self._matrix(self._like(a, "source", B, of), m) for a in source]
        if len({ld for _, ld in blocks}) > 1:
            blocks = [(a, ld) if ld == max(m, 1) else (self._start(a, B, of), max(m, 1)) for a, ld in blocks]
        return [a for a, _ in blocks], blocks[0][1]

    def _source_args(self, blocks, lds):
        """(nsrc, the array of the blocks' addresses or None, lds) as the scheduled exports take them."""
        if not blocks:
            return [0, None, lds]
        return [len(blocks), (C.c_void_p * len(blocks))(*[self._ptr(a) for a in blocks]), lds]

    def submatrix(self, rows, cols=None):
        """A[rows, cols] as a new resident operator of this class (otmb_op_submatrix; include/otmb.h states the contract): each argument a
        boolean mask (m entries for rows, n for cols) or an ascending 0-based index array; cols=None means rows again: the principal
        submatrix, which inherits the lines, restricted.  The child is the operator that would be made from SparseArrays' A[rows, cols]:
        stored order kept, values bit for bit, the parent's slots (each restricted) and selection.  Indices that do not ascend strictly or
        leave the matrix raise OtmbError, the message naming the first offending position; permutations and repeats are not built.  The caller
        owns the child; this operator is not modified."""
        self._live()
        m, n = self.shape
        r = self._selection(rows, m, "rows")
        c = r if cols is None else self._selection(cols, n, "cols")
        h = C.c_void_p()
        self.ctx.check(self._call("otmb_op_submatrix", int(r.shape[0]), self._ptr(r), int(c.shape[0]), self._ptr(c), C.byref(h)))
        return self._adopt(h)

    def take_values(self, parent, slot=None, parent_slot=None):
        """Slot `slot` of this operator -- a submatrix of `parent` -- becomes slot `parent_slot` of parent, restricted (otmb_op_take_values:
        one streaming launch on the device, nothing travels): the refresh after parent's values were rebuilt.  slot=None: the selected slot;
        parent_slot=None: the slot of the same number.  An operator that is not the parent this one was taken from raises OtmbError."""
        self._live()
        parent._live()
        slot = self.slots[1] if slot is None else int(slot)
        parent_slot = slot if parent_slot is None else int(parent_slot)
        self.ctx.check(self._library().otmb_op_take_values(self._h, parent._h, parent_slot, slot))

    def add_matrix(self, B, alpha=1.0, slots=None):
        """slot = slot + alpha·B in place (otmb_op_add_matrix; include/otmb.h states the contract) for a CSC matrix B of the operator's shape
        whose pattern lies inside the operator's -- the settling operator of buildTsink / DeviceAssembler.sinking added to a year of monthly
        T, or a diffusivity retuned without a rebuild (B = TκH, alpha = κ'/κ - 1).  B: an api.SparseMatrixCSC for api.DeviceOperator, a
        (colptr, rowval, nzval) triple of device tensors for device.Operator.  slots: None (every slot), an int, or a list of different slots.
        Each stored entry of B goes to the first stored entry of the operator with its row and column: nz = nz + (alpha * B), no FMA, the
        same bits into the row layout; entries B does not name are not rewritten; alpha == 0 checks the pattern and writes nothing.  An entry
        of B that the operator does not store raises OtmbError (PATTERN_NOT_CONTAINED, naming the first) and leaves every slot untouched.
        A submatrix child does not follow: child.take_values(self, slot) refreshes it."""
        self._live()
        m, n = self.shape
        cp, rv, nz = self._csc_arrays(B)
        if slots is None:
            nsel, sel = 0, None
        else:
            sel = np.ascontiguousarray(np.atleast_1d(np.asarray(slots)))
            if sel.ndim != 1 or not (np.issubdtype(sel.dtype, np.integer) or sel.size == 0):
                raise capi.OtmbError(11, f"invalid argument: slots must be None, an int or a list of ints, got {slots!r}")
            nsel = int(sel.size)
            sel = sel.astype(np.int64) if nsel else np.zeros(1, dtype=np.int64)  # (never a null pointer: that is "every slot")
        self.ctx.check(self._call("otmb_op_add_matrix", m, n, self._ptr(cp), self._ptr(rv), self._ptr(nz), float(alpha), nsel,
                                  None if sel is None else sel.ctypes.data))

    def to_csc(self, slot=None):
        """The operator's matrix as it was created (otmb_op_fetch): colptr, 1-based rowval and the nzval of slot `slot` (None: the selected
        one) -- an api.SparseMatrixCSC from api.DeviceOperator, three device tensors (colptr, rowval, nzval) from device.Operator."""
        self._live()
        if slot is not None and int(slot) < 0:
            raise capi.OtmbError(11, f"invalid argument: slot {slot}")
        cp, rv, nz = self._empty(self.shape[1] + 1, "int64"), self._empty(self.nnz, "int64"), self._empty(self.nnz, "float64")
        self.ctx.check(self._call("otmb_op_fetch", -1 if slot is None else int(slot), self._ptr(cp), self._ptr(rv), self._ptr(nz)))
        return self._csc(cp, rv, nz)

    @property
    def lines(self):
        """`next` as set_lines took it (otmb_op_get_lines: n int64 values, 1-based successors, 0 = none), or None when the operator has no lines."""
        self._live()
        nx, has = self._empty(self.shape[1], "int64"), C.c_int32(0)
        self.ctx.check(self._call("otmb_op_get_lines", self._ptr(nx), C.byref(has)))
        return nx if has.value else None

    def _info(self, h):
        """((m, n), nnz) of the operator behind the handle h."""
        m, n, z = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.ctx.check(self._library().otmb_op_info(h, C.byref(m), C.byref(n), C.byref(z)))
        return (int(m.value), int(n.value)), int(z.value)

    def precondition(self, Y, d=None, sigma=0.0, adjoint=False, precond="lines"):
        """Z = P⁻¹·Y with the preconditioner solve(..., precond=precond) uses for M = σ·I + diag(d) + A (adjoint: Aᵀ) (otmb_op_precond): for a
        Krylov method of the caller's own.  Y: 1-D or 2-D (n x k); d as in solve; returns a new Z of Y's shape (2-D: column-major)."""
        self._live()
        pc = capi.precond_code(precond)
        Y, k, Yc, ldy = self._state(Y, "Y")
        dc, dargs = self._d(d, Y, "Y")
        Z = self._zeros(tuple(Y.shape))
        name = "otmb_op_precond_dk" if len(dargs) == 2 else "otmb_op_precond"
        self.ctx.check(self._call(name, int(bool(adjoint)), pc, k, *dargs, float(sigma), self._ptr(Yc), ldy, self._ptr(Z), max(self.shape[0], 1)))
        return Z

    def solve(self, B, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False, precond="jacobi"):
        """X with (σ·I + diag(d) + A)·X = B (adjoint: ... + Aᵀ) by preconditioned BiCGStab on the device (otmb_op_solve_pc, include/otmb.h:
        the method, the stop rules, what is deterministic).  B: 1-D or 2-D (n x k); d: None (zero), n values, or a matrix of B's 2-D shape:
        every column has its own d (otmb_op_solve_dk); x0: None (start from zero) or an array of B's shape (not modified).  Returns (X, info):
        a new X of B's shape (2-D: column-major), info a SolveInfo with one entry per column (the call waits for the device to read it).  A
        column that does not converge is REPORTED (info.converged, info.reason), not raised: X then holds its last iterate.
        Argument errors and a zero or non-finite diagonal (SINGULAR_PRECONDITIONER) raise OtmbError.
        precond = "jacobi" (default) | "lines": the preconditioner; "lines" is P = M on the lines of set_lines (the water columns'
        tridiagonals: far fewer iterations on time-stepping systems) and needs set_lines first.  With "lines" only the pivots of
        the line factorisation are checked, not the diagonal: a zero or non-finite diag(M) entry is then reported, if it makes a pivot
        singular, as that pivot ("pivot[i] ...") -- also when next is all zero, where the results are Jacobi's but the message is not."""
        self._live()
        pc = capi.precond_code(precond)
        B, k, Bc, ldb = self._state(B, "B")
        dc, dargs = self._d(d, B, "B")
        X = self._start(x0, B, "B")
        iters, relres, reason = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.int32)
        name = "otmb_op_solve_dk" if len(dargs) == 2 else "otmb_op_solve_pc"
        rc = self._call(name, int(bool(adjoint)), k, *dargs, float(sigma), self._ptr(Bc), ldb, self._ptr(X), max(self.shape[0], 1), int(x0 is not None),
                        float(rtol), int(maxiter), iters.ctypes.data, relres.ctypes.data, reason.ctypes.data, pc)
        return X, SolveInfo(self._status(rc), iters, relres, reason)

    def observe(self, W, X):
        """Wᵀ·X on the device (otmb_op_observe; include/otmb.h states the order of the sums): W n x q (or n values: one observer), X n x k or
        1-D.  Returns a new array (q, k), or (q,) for 1-D X: inventories (W = the cell volumes), stations, regional means of a state.  On
        device tensors it is enqueued on the context's stream and nothing travels to the host."""
        self._live()
        n = self.shape[1]
        X = self._array(X, "X")
        if X.ndim not in (1, 2) or X.shape[0] != n:
            raise capi.OtmbError(11, f"DimensionMismatch: operator of {self.shape}, X of {tuple(X.shape)}")
        k = 1 if X.ndim == 1 else X.shape[1]
        Xc, ldx = self._matrix(X, n)
        W, q = observers(self._array(W, "observe"), n)
        Wc, ldw = self._matrix(W, n)
        obs = self._zeros((q, k))
        self.ctx.check(self._call("otmb_op_observe", k, q, self._ptr(Wc), ldw, self._ptr(Xc), ldx, self._ptr(obs)))
        return obs[:, 0] if X.ndim == 1 else obs

    def step(self, X, *, dt, theta=1.0, nsteps=1, first_slot=0, source=None, d=None, rtol=1e-10, maxiter=10000, adjoint=False, precond="jacobi",
             observe=None, time_weights=None):
        """nsteps θ-steps of ∂x/∂t + (diag(d) + A)·x = source from the state X, step t with the matrix of slot (first_slot + t) mod nslots
        (otmb_op_step; include/otmb.h states the contract: σ = 1 / (theta·dt), the right-hand side, then solve(..., x0 = the state)).  X: 1-D
        or 2-D (n x k), not modified: the steps run on a copy; source: None (zero) or an array of X's shape; d: None, n values, or a matrix of
        X's 2-D shape: every tracer has its own d (otmb_op_step_dk), and column c is the 1-D call with d[:, c].  Returns (X after the steps,
        info): info a StepInfo.  A step that does not converge ends the call and is REPORTED as solve reports it (info.status,
        info.steps_done, info.reason; X then holds that step's last iterates), not raised; argument errors and a singular preconditioner
        raise OtmbError.  Nothing but the solver's column records travels to the host.
        observe: W, n x q (or n values: one observer) -> info.observations, (steps_done, k, q); time_weights: nsteps finite host values ->
        info.mean = Σ_t time_weights[t]·X_t, n x k.  With either the call is otmb_op_step_obs (include/otmb.h states the order of the sums
        and the mean's fold); with neither it is the plain one, and info.observations and info.mean are None.
        source may also be a list or tuple of arrays of X's shape, one (every step takes it) or one per slot (step t takes the block of its
        slot: the source of the month): the call is then step_sched's, which also has sub-steps and a history."""
        return self.step_sched(X, dt=dt, theta=theta, nsteps=nsteps, first_slot=first_slot, source=source, d=d, rtol=rtol, maxiter=maxiter,
                               adjoint=adjoint, precond=precond, observe=observe, time_weights=time_weights)

    def step_sched(self, X, *, dt, theta=1.0, nsteps=1, first_slot=0, substeps=1, source=None, source_scale=None, d=None, rtol=1e-10, maxiter=10000,
                   adjoint=False, precond="jacobi", observe=None, time_weights=None):
        """step with a schedule for the time axis (otmb_op_step_sched; include/otmb.h states the contract).  substeps = m >= 1: step t runs
        with slot (first_slot + t // m) mod nslots -- m implicit steps inside January before February begins; each slot's preconditioner is
        made once and reused by its sub-steps.  source: None, an array of X's shape, or a list or tuple of such arrays, one (every step) or one
        per slot (step t takes its slot's: a seasonal source); for device.Operator the blocks are separate tensors, and nothing is stacked.
        source_scale: None, or host values of shape (nsteps, k) -- (nsteps,) for a 1-D X --: the source of step t and tracer c is
        source·source_scale[t, c], a fixed pattern times a history (CFC-11, SF6, bomb radiocarbon).  Step t has the bits of step(nsteps=1,
        first_slot=its slot, source=source·source_scale[t]) from the state before it.  Everything else, and what is returned, is step's;
        with substeps=1, a single array and no source_scale the call IS step's, made through the same exports."""
        self._live()
        pc = capi.precond_code(precond)
        X, k, Xc, _ = self._state(X, "X")
        dc, dargs = self._d(d, X, "X")
        Sc, lds, blocks = None, max(self.shape[0], 1), None
        if isinstance(source, (list, tuple)):
            blocks, lds = self._sources(source, X, "X")
        elif source is not None:
            Sc, lds = self._matrix(self._like(source, "source", X, "X"), self.shape[0])
        sched = blocks is not None or source_scale is not None or int(substeps) != 1
        if sched:  # the schedule in place of S, lds; one d for every tracer is ldd = 0
            dargs = dargs if len(dargs) == 2 else dargs + [0]
        record = sched or len(dargs) == 2 or observe is not None or time_weights is not None
        name = "otmb_op_step_sched" if sched else "otmb_op_step_dk" if len(dargs) == 2 else "otmb_op_step_obs" if record else "otmb_op_step"
        return self._step_call(name, X, k, Xc, dargs, nsteps, [int(first_slot), int(substeps)] if sched else [int(first_slot)],
                               ([] if Sc is None else [Sc]) if blocks is None else blocks, lds, dt=dt, theta=theta, source_scale=source_scale, rtol=rtol,
                               maxiter=maxiter, adjoint=adjoint, pc=pc, observe=observe, time_weights=time_weights, listed=sched, record=record)

    def _step_call(self, name, X, k, Xc, dargs, nsteps, sched_args, blocks, lds, *, dt, theta, source_scale, rtol, maxiter, adjoint, pc, observe,
                   time_weights, listed=True, record=True):
        """What every step method does once its d (dargs), its schedule (sched_args, behind nsteps in the export's list) and its source blocks
        are marshalled: the scale, the observers and the mean's weights, the copy of the state, the report arrays, the call and its StepInfo.
        listed: the source goes as nsrc, S, lds, scale (the scheduled exports), otherwise as S, lds; record: the export takes the observers."""
        n, ld = self.shape[1], max(self.shape[0], 1)
        scale = None
        if source_scale is not None:
            if not blocks:
                raise capi.OtmbError(11, "invalid argument: source_scale needs a source")
            scale = np.ascontiguousarray(source_scale, dtype=np.float64)
            want = (max(int(nsteps), 0),) + tuple(X.shape[1:])
            if scale.shape != want:
                raise capi.OtmbError(11, f"DimensionMismatch: source_scale of {scale.shape}, expected {want}")
        q, Wc, ldw, obs, tw, mean = 0, None, max(n, 1), None, None, None
        if observe is not None:
            W, q = observers(self._array(observe, "observe"), n)
            Wc, ldw = self._matrix(W, n)
            obs = self._zeros((max(int(nsteps), 0), k, q), "C")
        if time_weights is not None:
            tw = _as_weights(time_weights, nsteps)
            mean = self._zeros(tuple(X.shape))
        Xn = self._zeros(tuple(X.shape))
        self._assign(Xn, Xc)
        iters, relres, reason = step_arrays(nsteps, k)
        done = C.c_int64(0)
        if listed:
            sargs = [*self._source_args(blocks, lds), None if scale is None else scale.ctypes.data]
        else:
            sargs = [self._ptr(blocks[0] if blocks else None), lds]
        args = [int(bool(adjoint)), k, *dargs, float(dt), float(theta), int(nsteps), *sched_args, *sargs, self._ptr(Xn), ld, float(rtol), int(maxiter), pc,
                C.byref(done), iters.ctypes.data, relres.ctypes.data, reason.ctypes.data]
        if record:  # the record's arguments; q = 0 and nulls make the per-column call the plain step
            args += [q, self._ptr(Wc), ldw, self._ptr(obs), None if tw is None else tw.ctypes.data, self._ptr(mean), ld]
        rc = self._call(name, *args)
        return Xn, StepInfo(self._status(rc), done.value, nsteps, iters, relres, reason, obs, mean)

    def _interp(self, slot_a, slot_b, weight):
        """The interpolated schedule as the exports take it: (slot_a, slot_b as int64, weight as float64 host arrays of one length, that
        length).  Integer slots of the operator and finite weights in [0, 1] only: refused here, before the library is called."""
        arrays = []
        for name, a in (("slot_a", slot_a), ("slot_b", slot_b)):
            a = np.asarray(a)
            if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
                raise capi.OtmbError(11, f"invalid argument: {name} must be a 1-D array of integers, got {a.dtype} of {a.shape}")
            arrays.append(np.ascontiguousarray(a, dtype=np.int64))
        w = np.asarray(weight)
        if w.ndim != 1 or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer) or w.size == 0):
            raise capi.OtmbError(11, f"invalid argument: weight must be a 1-D array of real numbers, got {w.dtype} of {w.shape}")
        w = np.ascontiguousarray(w, dtype=np.float64)
        a, b = arrays
        if not (a.shape == b.shape == w.shape):
            raise capi.OtmbError(11, f"DimensionMismatch: slot_a of {a.shape}, slot_b of {b.shape}, weight of {w.shape}")
        nslots = self.slots[0]
        for name, s in (("slot_a", a), ("slot_b", b)):
            if s.size and (s.min() < 0 or s.max() >= nslots):
                raise capi.OtmbError(11, f"invalid argument: {name} holds a slot outside 0..{nslots - 1}")
        if w.size and not (np.isfinite(w).all() and w.min() >= 0.0 and w.max() <= 1.0):
            raise capi.OtmbError(11, "invalid argument: weight must be finite and in [0, 1]")
        return a, b, w, int(w.shape[0])

    def _one_source(self, source):
        """The source of the interpolated calls as they take it -- None, an array, or a list or tuple of ONE -- without its wrapping."""
        if isinstance(source, (list, tuple)):
            if len(source) != 1:
                raise capi.OtmbError(11, f"DimensionMismatch: {len(source)} source blocks, expected 1 (a source per slot is not built with interpolation)")
            source = source[0]
        return source

    def step_interp(self, X, *, dt, slot_a, slot_b, weight, theta=1.0, source=None, source_scale=None, d=None, rtol=1e-10, maxiter=10000,
                    adjoint=False, precond="jacobi", observe=None, time_weights=None):
        """step with the matrices interpolated between slots (otmb_op_step_interp; include/otmb.h states the contract): step t runs with
        (1 - weight[t])·(slot slot_a[t]) + weight[t]·(slot slot_b[t]) -- the slot itself where the two are one or the weight is 0 or 1.  The
        three 1-D host arrays have one length, which is the number of steps; interp_schedule (api.py) makes them for the TMM convention
        (monthly means valid at mid-month).  source: None, an array of X's shape, or a list of one; source_scale, d, observe, time_weights
        and what is returned are step_sched's.  A blended step has the bits of combine_slots into a spare slot followed by step(nsteps=1)
        on it; its preconditioner is made afresh, which is the cost of the convention."""
        self._live()
        pc = capi.precond_code(precond)
        X, k, Xc, _ = self._state(X, "X")
        dc, dargs = self._d(d, X, "X")
        sa, sb, w, nsteps = self._interp(slot_a, slot_b, weight)
        source = self._one_source(source)
        Sc, lds = (None, max(self.shape[0], 1)) if source is None else self._matrix(self._like(source, "source", X, "X"), self.shape[0])
        return self._step_call("otmb_op_step_interp", X, k, Xc, dargs if len(dargs) == 2 else dargs + [0], nsteps, [sa.ctypes.data, sb.ctypes.data, w.ctypes.data],
                               [] if Sc is None else [Sc], lds, dt=dt, theta=theta, source_scale=source_scale, rtol=rtol, maxiter=maxiter, adjoint=adjoint, pc=pc,
                               observe=observe, time_weights=time_weights)

    def periodic_interp(self, source, *, dt, slot_a, slot_b, weight, theta=1.0, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False,
                        precond="jacobi", ptol=1e-8, restart=30, maxcycles=1000, outer="none"):
        """periodic over a cycle of interpolated steps (otmb_op_periodic_interp; include/otmb.h): F is step_interp over the schedule, whose
        length is the cycle's number of steps; source: an array, or a list of one.  With outer="mean" the mean's weights are the slots'
        shares of the schedule's weights.  No source_scale: a history is not periodic.  Everything else, and what is returned, is
        periodic's."""
        oc = capi.outer_code(outer)
        self._live()
        pc = capi.precond_code(precond)
        S, k, Sc, lds = self._state(self._one_source(source), "source")
        sa, sb, w, ncycle = self._interp(slot_a, slot_b, weight)
        dc, dargs = self._d(d, S, "source")
        return self._periodic_call("otmb_op_periodic_interp", S, k, dargs if len(dargs) == 2 else dargs + [0], ncycle, [sa.ctypes.data, sb.ctypes.data, w.ctypes.data],
                                   self._source_args([Sc], lds), dt=dt, theta=theta, x0=x0, rtol=rtol, maxiter=maxiter, adjoint=adjoint, pc=pc, ptol=ptol,
                                   restart=restart, maxcycles=maxcycles, oc=oc)

    def _ds(self, d, B, what):
        """(what keeps the blocks alive, [nd, the array of the blocks' addresses or None, ldd]) of the season calls' d: None, n values, an array
        of the state's shape, or a list or tuple of one or nslots such arrays of one shape -- n values each (ldd = 0: they serve every column)
        or of B's 2-D shape (column c is tracer c's).  Blocks whose leading dimensions differ are copied compactly; nothing is stacked."""
        if d is None:
            return None, [0, None, 0]
        blocks = list(d) if isinstance(d, (list, tuple)) else [d]
        nslots = self.slots[0]
        if len(blocks) not in (1, nslots):
            raise capi.OtmbError(11, f"DimensionMismatch: {len(blocks)} d blocks, expected 1 or one per slot ({nslots})")
        blocks = [self._array(a, "d") for a in blocks]
        if len({tuple(a.shape) for a in blocks}) > 1:
            raise capi.OtmbError(11, f"DimensionMismatch: d blocks of different shapes: {sorted({tuple(a.shape) for a in blocks})}")
        n = self.shape[1]
        if blocks[0].ndim != 2:
            for a in blocks:
                self._check_d(a, (n,), what)
            kept = [self._matrix(a, n)[0] for a in blocks]
            return kept, [len(kept), (C.c_void_p * len(kept))(*[self._ptr(a) for a in kept]), 0]
        if B.ndim != 2:
            raise capi.OtmbError(11, f"DimensionMismatch: d of {tuple(blocks[0].shape)} is per column, {what} of {tuple(B.shape)} has no columns")
        for a in blocks:
            self._check_d(a, tuple(B.shape), what)
        pairs = [self._matrix(a, n) for a in blocks]
        if len({ld for _, ld in pairs}) > 1:
            pairs = [(a, ld) if ld == max(n, 1) else (self._start(a, B, what), max(n, 1)) for a, ld in pairs]
        kept = [a for a, _ in pairs]
        return kept, [len(kept), (C.c_void_p * len(kept))(*[self._ptr(a) for a in kept]), pairs[0][1]]

    def _season_sources(self, source, B, of):
        """(the source blocks column-major, lds) of the season calls: None, an array of B's shape, or a list or tuple of one or nslots."""
        if source is None:
            return [], max(self.shape[0], 1)
        if not isinstance(source, (list, tuple)):
            Sc, lds = self._matrix(self._like(source, "source", B, of), self.shape[0])
            return [Sc], lds
        if not source:
            raise capi.OtmbError(11, "DimensionMismatch: 0 source blocks, expected 1 or one per slot")
        return self._sources(source, B, of)

    def _periodic_sources(self, source):
        """(the first block as given, k, it column-major, the blocks' lds, the blocks column-major) of a periodic call's source: an array of
        the state's shape, or a list or tuple of one or nslots such arrays."""
        if not isinstance(source, (list, tuple)):
            S, k, Sc, lds = self._state(source, "source")
            return S, k, Sc, lds, [Sc]
        if not source:
            raise capi.OtmbError(11, "DimensionMismatch: 0 source blocks, expected 1 or one per slot")
        S, k, Sc, _ = self._state(source[0], "source")
        blocks, lds = self._sources(source, S, "source")
        return S, k, Sc, lds, blocks

    def step_season(self, X, *, dt, slot_a, slot_b, weight, theta=1.0, d=None, source=None, source_scale=None, rtol=1e-10, maxiter=10000,
                    adjoint=False, precond="jacobi", observe=None, time_weights=None):
        """step_interp with d and the source per slot as well (otmb_op_step_season; include/otmb.h states the contract): every per-step field
        follows the calendar the way the matrix does.  d: None, n values, an array of X's shape, or a list or tuple of one or nslots such
        arrays of one shape; source: None, an array of X's shape, or a list or tuple of one or nslots.  A field given once serves every
        step as it is.  A field given per slot is the slot's block on a plain step and (1 - weight[t])·(block slot_a[t]) +
        weight[t]·(block slot_b[t]) on a blended one, folded as the matrix is; source_scale then multiplies the blended source.  With
        plain_schedule (api.py) the explicit schedule is step_sched's.  Step t has the bits of combine_slots into a spare slot followed by
        step(nsteps=1) with that step's d and source.  Everything else, and what is returned, is step_interp's."""
        self._live()
        pc = capi.precond_code(precond)
        X, k, Xc, _ = self._state(X, "X")
        dkeep, dargs = self._ds(d, X, "X")
        sa, sb, w, nsteps = self._interp(slot_a, slot_b, weight)
        blocks, lds = self._season_sources(source, X, "X")
        return self._step_call("otmb_op_step_season", X, k, Xc, dargs, nsteps, [sa.ctypes.data, sb.ctypes.data, w.ctypes.data], blocks, lds, dt=dt, theta=theta,
                               source_scale=source_scale, rtol=rtol, maxiter=maxiter, adjoint=adjoint, pc=pc, observe=observe, time_weights=time_weights)

    def periodic_season(self, source, *, dt, slot_a, slot_b, weight, theta=1.0, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False,
                        precond="jacobi", ptol=1e-8, restart=30, maxcycles=1000, outer="none"):
        """periodic over a cycle of step_season's steps (otmb_op_periodic_season; include/otmb.h): the cyclo-stationary state under a seasonal
        d and a seasonal source.  source: an array, or a list or tuple of one or nslots arrays of one shape; d: as in step_season.  A column is
        answered with zero only when it is zero in every source block.  With outer="mean" the mean operator is diag(d̄) + Ā, d̄ the fold of
        the d blocks under the mean's own weights; it changes only how fast the iteration converges.  No source_scale: a history is not
        periodic.  Everything else, and what is returned, is periodic_interp's."""
        oc = capi.outer_code(outer)
        self._live()
        pc = capi.precond_code(precond)
        S, k, Sc, lds, blocks = self._periodic_sources(source)
        sa, sb, w, ncycle = self._interp(slot_a, slot_b, weight)
        dkeep, dargs = self._ds(d, S, "source")
        return self._periodic_call("otmb_op_periodic_season", S, k, dargs, ncycle, [sa.ctypes.data, sb.ctypes.data, w.ctypes.data], self._source_args(blocks, lds),
                                   dt=dt, theta=theta, x0=x0, rtol=rtol, maxiter=maxiter, adjoint=adjoint, pc=pc, ptol=ptol, restart=restart, maxcycles=maxcycles,
                                   oc=oc)

    def periodic(self, source, *, dt, ncycle, theta=1.0, first_slot=0, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False, precond="jacobi",
                 ptol=1e-8, restart=30, maxcycles=1000, outer="none"):
        """The periodic state of the stepped cycle: X with F(X) = X, F = step(..., nsteps=ncycle, first_slot=first_slot, source=source), by
        restarted GMRES(restart) on the cycle map (otmb_op_periodic; include/otmb.h states the method and what is deterministic).  source:
        1-D or 2-D (n x k); x0: None (start from zero) or an array of source's shape (not modified); d: None, n values, or a matrix of
        source's 2-D shape: every column has its own d (otmb_op_periodic_dk); the other arguments are step's.  Returns (X, info): a new X,
        the state at the start of the cycle, with ‖F(X) - X‖₂ <= ptol·‖F(0)‖₂ per converged column, info a PeriodicInfo.  A column that
        does not converge is REPORTED (info.reason), not raised; argument errors and a singular preconditioner raise OtmbError.  Per round
        the host reads a few scalars a column; no vector travels.
        outer = "none" (default) | "mean": with "mean" the outer GMRES is flexible and preconditioned by the cycle-mean operator
        (otmb_op_periodic_pc with OTMB_OUTER_MEAN; include/otmb.h states the method) -- fewer cycles, one solve with the mean matrix per
        iteration (info.msolve_iters; zero with "none").
        source may also be a list or tuple of arrays of one shape, one or one per slot: the call is then periodic_sched's."""
        return self.periodic_sched(source, dt=dt, ncycle=ncycle, theta=theta, first_slot=first_slot, d=d, x0=x0, rtol=rtol, maxiter=maxiter,
                                   adjoint=adjoint, precond=precond, ptol=ptol, restart=restart, maxcycles=maxcycles, outer=outer)

    def periodic_sched(self, source, *, dt, ncycle, theta=1.0, first_slot=0, substeps=1, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False,
                       precond="jacobi", ptol=1e-8, restart=30, maxcycles=1000, outer="none"):
        """periodic with a schedule (otmb_op_periodic_sched; include/otmb.h): F is step_sched over ncycle steps with `substeps` and `source`,
        an array or a list or tuple of arrays of one shape, one or one per slot (a seasonal source; the cycle map stays affine).  A column is
        answered with zero only when it is zero in every block; with outer="mean" the mean's weights are the slots' shares of the cycle's
        steps.  No source_scale: a history is not periodic.  Everything else, and what is returned, is periodic's; with substeps=1 and a
        single array the call IS periodic's, made through the same exports."""
        oc = capi.outer_code(outer)
        self._live()
        pc = capi.precond_code(precond)
        S, k, Sc, lds, blocks = self._periodic_sources(source)
        sched = isinstance(source, (list, tuple)) or int(substeps) != 1
        dc, dargs = self._d(d, S, "source")
        if sched:  # the schedule in place of S, lds; one d for every column is ldd = 0
            dargs = dargs if len(dargs) == 2 else dargs + [0]
            sargs = [int(first_slot), int(substeps), *self._source_args(blocks, lds)]
        else:
            sargs = [int(first_slot), self._ptr(Sc), lds]
        outer_args = sched or len(dargs) == 2 or oc != capi.OUTERS["none"]
        name = "otmb_op_periodic_sched" if sched else "otmb_op_periodic_dk" if len(dargs) == 2 else "otmb_op_periodic_pc" if outer_args else "otmb_op_periodic"
        return self._periodic_call(name, S, k, dargs, ncycle, sargs, [], dt=dt, theta=theta, x0=x0, rtol=rtol, maxiter=maxiter, adjoint=adjoint, pc=pc, ptol=ptol,
                                   restart=restart, maxcycles=maxcycles, oc=oc, outer_args=outer_args)

    def _periodic_call(self, name, S, k, dargs, ncycle, sched_args, source_args, *, dt, theta, x0, rtol, maxiter, adjoint, pc, ptol, restart, maxcycles, oc,
                       outer_args=True):
        """What every periodic method does once its source (S: the state-shaped first block), its d, its schedule and its source arguments
        (sched_args, source_args: behind ncycle in the export's list) are marshalled: the start, the report arrays, the call and its
        PeriodicInfo.  outer_args: the export takes outer and msolve_iters."""
        X = self._start(x0, S, "source")
        cycles, defect, reason = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.float64), np.zeros(k, dtype=np.int32)
        args = [int(bool(adjoint)), k, *dargs, float(dt), float(theta), int(ncycle), *sched_args, *source_args, self._ptr(X), max(self.shape[0], 1),
                int(x0 is not None), float(rtol), int(maxiter), pc, float(ptol), int(restart), int(maxcycles), cycles.ctypes.data, defect.ctypes.data,
                reason.ctypes.data]
        msolve = None
        if outer_args:
            msolve = np.zeros(k, dtype=np.int64)
            args += [oc, msolve.ctypes.data]
        rc = self._call(name, *args)
        return X, PeriodicInfo(self._status(rc), cycles, defect, reason, msolve)
