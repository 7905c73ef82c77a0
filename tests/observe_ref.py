"""A numpy restatement of otmb_op_observe and of the record of otmb_op_step_obs (csrc/otmb_observe.hip, include/otmb.h): obs[j, c] =
Σ_i W[i, j]·X[i, c] in the device's order, and the mean's fold Xbar = Σ_t tw[t]·X_t.

The order: a workgroup of 256 lanes takes OB_ROWS = 2048 rows; lane t takes the row pairs starting at rows 2·(1024·wg + t + 256·p), p = 0..3;
its accumulator starts at +0.0 and takes the product of the pair's first row, then of the second (one multiplication, one addition each);
the workgroup's tree is csrc/otmb_op_sum.h's (xor shuffles 32..1 inside a wave of 64, then the four waves in order); an entry's partials are
added in workgroup order from partial 0.  Rows at and beyond n are not read on the device; here they add +0.0, which changes no bit: an
accumulator that began at +0.0 is never -0.0."""
import numpy as np

OB_ROWS = 2048  # csrc/otmb_observe.hip
LANE_ADDS, SHUFFLES, WAVE_ADDS = 8, 6, 3  # the roundings a term can pass through inside one workgroup


def workgroups(n):
    return (n + OB_ROWS - 1) // OB_ROWS


def roundings(n):
    """The most additions any product passes through on its way into a sum over n rows."""
    return LANE_ADDS + SHUFFLES + WAVE_ADDS + max(workgroups(n) - 1, 0)


def device_sums(prod):
    """Σ over axis 0 of prod (n, ...) in the device's order: every trailing index is a sum of its own."""
    prod = np.asarray(prod, dtype=np.float64)
    n, rest = prod.shape[0], prod.shape[1:]
    nwg = workgroups(n)
    if nwg == 0:
        return np.zeros(rest)
    p = np.zeros((nwg * OB_ROWS,) + rest)
    p[:n] = prod
    p = p.reshape((nwg, OB_ROWS // 512, 256, 2) + rest)
    acc = np.zeros((nwg, 256) + rest)
    for q in range(OB_ROWS // 512):  # a lane's pairs, each pair's two rows in order
        acc = acc + p[:, q, :, 0]
        acc = acc + p[:, q, :, 1]
    x = acc.reshape((nwg, 4, 64) + rest)  # op_block_sum: the shuffles of a wave, then the waves in order
    lane = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, lane ^ dist]
    s = x[:, :, 0]
    part = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
    out = part[0]  # the fold: workgroup order from partial 0
    for b in range(1, nwg):
        out = out + part[b]
    return out


def observe_ref(W, X):
    """obs (q, k) of W (n, q) and X (n, k)."""
    W, X = np.asarray(W, dtype=np.float64), np.asarray(X, dtype=np.float64)
    W = W.reshape(W.shape[0], 1) if W.ndim == 1 else W
    X = X.reshape(X.shape[0], 1) if X.ndim == 1 else X
    with np.errstate(invalid="ignore", over="ignore"):
        return device_sums(W[:, :, None] * X[:, None, :])


def mean_ref(states, tw):
    """The mean's fold over the completed steps' states: +0.0 + tw[0]·X_0, then + tw[t]·X_t, the product first."""
    Xbar = None
    for t, X in enumerate(states):
        P = tw[t] * np.asarray(X, dtype=np.float64)
        Xbar = (0.0 + P) if Xbar is None else Xbar + P
    return Xbar


def flat_sum(prod):
    """Σ prod left to right from +0.0: NOT the device's order."""
    s = 0.0
    for v in prod:
        s = s + float(v)
    return s


def same_values(a, b):
    """Bit for bit, except that any NaN equals any NaN (a NaN's sign and payload are the processor's choice, not the order's)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a[~na]).view(np.uint64), np.ascontiguousarray(b[~nb]).view(np.uint64)))
