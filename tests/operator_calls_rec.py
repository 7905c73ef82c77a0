"""What tests/test_operator_calls_host.py and tests/test_operator_calls_dev.py share: a recorder that stands in for the loaded library, a context
that records what it is asked to check, and the arguments of a recorded call under the names include/otmb.h gives them -- so that "the
header's order" is read from the header, not restated."""
import re

from test_julia_shim_static import HEADER, split_top

N, K = 6, 3


def _scalars(adjoint, precond, code):
    """(the keywords of the Python methods, the values include/otmb.h's names must then hold).  These integers are unlike the others of a
    call -- k is 1 or 3, nsteps 2, the leading dimensions 6 or 8, q at most 2 -- so none can stand in another's place."""
    common = dict(dt=0.25, theta=0.5, first_slot=11, rtol=1e-7, maxiter=77)
    return dict(common, adjoint=adjoint, precond=precond), dict(common, adjoint=int(adjoint), precond=code)


# the two flags that are 0 or 1, the adjoint and the otmb_precond code, never have the same value in one call: swapped, they would show
CASES = [_scalars(True, "jacobi", 0), _scalars(False, "lines", 1)]
CASE_IDS = ["adjoint-jacobi", "plain-lines"]
PERIODIC = dict(ncycle=4, ptol=1e-5, restart=9, maxcycles=55)


def only(d, *keys):
    return {k: d[k] for k in keys}


def header_names(name):
    """The parameter names of an export's prototype in include/otmb.h, in order."""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    args = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", text).group(1)
    return [re.search(r"(\w+)\s*$", a).group(1) for a in split_top(" ".join(args.split()))]
SIGNATURES = {
    "precondition": "(self, Y, d=None, sigma=0.0, adjoint=False, precond='lines')",
    "solve": "(self, B, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False, precond='jacobi')",
    "observe": "(self, W, X)",
    "step": "(self, X, *, dt, theta=1.0, nsteps=1, first_slot=0, source=None, d=None, rtol=1e-10, maxiter=10000, adjoint=False, "
            "precond='jacobi', observe=None, time_weights=None)",
    "periodic": "(self, source, *, dt, ncycle, theta=1.0, first_slot=0, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False, "
                "precond='jacobi', ptol=1e-08, restart=30, maxcycles=1000, outer='none')",
}


class Recorder:
    """Every export is a function that records (name, arguments) and returns `rc`."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if not name.startswith("otmb_"):
            raise AttributeError(name)

        def export(*args):
            self.calls.append((name, args))
            return self.rc

        return export


class Ctx:
    def __init__(self):
        self.checked = []

    def check(self, rc):
        self.checked.append(rc)


def host_operator(monkeypatch, rc=0):
    """(an api.DeviceOperator of N x N without a context or a device, the recorder its calls reach in place of the library)."""
    import ctypes as C

    from otmb_amd import api, capi

    rec = Recorder(rc)
    monkeypatch.setattr(capi, "lib", lambda: rec)
    D = api.DeviceOperator.__new__(api.DeviceOperator)  # (the methods under test only read these)
    D._h, D.shape, D.ctx = C.c_void_p(1), (N, N), Ctx()
    D.close = lambda: None  # (its handle is no operator's: there is nothing to destroy when it goes)
    return D, rec


def the_call(rec, name):
    """The arguments of the ONE call recorded since the last look, by the header's names; its export is `name`, its length the mirror's."""
    from otmb_amd import capi

    assert [n for n, _ in rec.calls] == [name]
    args = rec.calls.pop()[1]
    names = header_names(name)
    assert len(args) == len(capi.SYMBOLS[name][1]) == len(names), name
    return dict(zip(names, args))


def has(a, **want):
    """Every named argument has the value, and the value's type (1 is not 1.0 to a ctypes prototype's reader, None is the null pointer)."""
    for key, value in want.items():
        assert a[key] == value and type(a[key]) is type(value), (key, a[key], value)
