"""Two grids between the unit cases (at most 26 fill tiles) and the 1 degree grid (11 920): the smallest on which the fill pass, the tile scans
and the T fix-up work across MORE THAN ONE SCAN GROUP (otmb_scan.hip: 1024 tiles to a group; a fill tile is 256 wet columns, a makeindices /
tfix tile 1024 cells / columns, a sparse() tile 256 sorted entries).

  "mid"   328 x 100 x 17  ~340 000 wet cells: two scan groups of fill tiles, a seam row that is dealt round the eight XCDs more than once, tiles
          of two to three grid rows (a cell's south / north neighbours lie in other tiles), an odd nz, the pair kernel of facefluxes;
  "wide"  1040 x 512 x 4  ~1.2 M wet cells: five scan groups of fill tiles, three of makeindices, two of tfix; nx * ny >= 2^19 with nx >= 512 is
          the four-row geometry of facefluxes by itself.

Both are synthetic.make_grid(..., seed=78, rho="array").  Beside the grids: transport fields whose signs and sizes change from step to step
(the rule of test_kept_ops._fields), fields without an exact zero and one with every fifth transport zeroed (test_kept_t_pattern._cancel_fields),
a Float32 copy, and the oracle's results, computed once per (grid, field, ρ, κ, weighting) and left unchanged.  tests/test_mid_grids_ref.py asserts
on the CPU that the grids are what tests/test_mid_grids.py needs."""
import numpy as np

from helpers import MATS, gridmetrics_of
from otmb_amd import synthetic

SHAPES = {"mid": (328, 100, 17), "wide": (1040, 512, 4)}
SEED = 78
TILE = 256            # wet columns per fill tile (TM_TILE)
SCAN_GROUP = 1024     # tiles per scan group (OTMB_SCAN_GROUP)
BIG_TILE = 1024       # cells per makeindices tile, columns per tfix tile
RHO_SCALAR = 1035.0

_grids, _fields, _phi, _tm = {}, {}, {}, {}


def case(name):
    """(grid, gridmetrics) of "mid" / "wide": built once and left unchanged."""
    if name not in _grids:
        g = synthetic.make_grid(*SHAPES[name], seed=SEED, rho="array")
        _grids[name] = (g, gridmetrics_of(g))
    return _grids[name]


def wet_mask(name):
    g, gm = case(name)
    return ~np.isnan(np.asarray(gm.v3D))


def fill_value(name):
    return case(name)[0].umo.properties["_FillValue"]


def kappa(name, kind="grid"):
    """"grid": the grid's own three; "noH": κH = 0 (explicit zeros in TκH: T's horizontal rows cancel where no flux passes); "other": another κH and
    κVdeep (a given operator with the derived rows and other values)."""
    g = case(name)[0]
    return {"grid": (g.kappaH, g.kappaVML, g.kappaVdeep), "noH": (0.0, g.kappaVML, g.kappaVdeep), "other": (123.0, g.kappaVML, 7.5e-5)}[kind]


def field(name, which):
    """(umo, vmo, fill): 3-D column-major host arrays, land at the fill value.
    "base": the grid's own transports; "step0" .. "step2": base times factors from -1.5 .. 1.5 drawn per step, the third with every fifth umo
    zeroed (test_kept_ops._fields); "plain0", "plain1": ±(0.5 .. 1.5), no exact zero on any face; "cancel": likewise with every fifth transport
    zeroed (test_kept_t_pattern._cancel_fields); "f32": step0 rounded to Float32."""
    key = (name, which)
    if key in _fields:
        return _fields[key]
    g, gm = case(name)
    wet = wet_mask(name)
    fill = fill_value(name)
    u0, v0 = np.asarray(g.umo.data), np.asarray(g.vmo.data)
    G = wet.size

    def land(x):
        return np.asfortranarray(np.where(wet, x.reshape(wet.shape, order="F"), fill))

    if which == "base":
        out = (np.asfortranarray(u0), np.asfortranarray(v0), fill)
    elif which.startswith("step"):
        k = int(which[4:])
        rng = np.random.default_rng([SEED, 1, k])
        fu, fv = rng.uniform(-1.5, 1.5, G), rng.uniform(-1.5, 1.5, G)
        if k % 3 == 2:
            fu[::5] = 0.0
        out = (land(u0.ravel(order="F") * fu), land(v0.ravel(order="F") * fv), fill)
    elif which in ("plain0", "plain1", "cancel"):
        rng = np.random.default_rng([SEED, 2, ("plain0", "plain1", "cancel").index(which)])
        pair = []
        for _ in range(2):
            f = rng.uniform(0.5, 1.5, G) * rng.choice([-1.0, 1.0], G)
            if which == "cancel":
                f[::5] = 0.0
            pair.append(land(f))
        out = (pair[0], pair[1], fill)
    elif which == "f32":
        u, v, _ = field(name, "step0")
        f32 = float(np.float32(fill))
        out = (np.asfortranarray(np.where(wet, u, f32).astype(np.float32)), np.asfortranarray(np.where(wet, v, f32).astype(np.float32)), f32)
    else:
        raise KeyError(which)
    for a in out[:2]:
        a.setflags(write=False)
    _fields[key] = out
    return out


def indices(oracle, name):
    key = (name, "idx")
    if key not in _phi:
        _phi[key] = oracle.makeindices(case(name)[1].v3D)
    return _phi[key]


def facefluxes(oracle, name, which):
    """The oracle's six ϕ of a field (cached)."""
    key = (name, which)
    if key not in _phi:
        g, gm = case(name)
        u, v, fill = field(name, which)
        _phi[key] = oracle.facefluxes(u, v, indices(oracle, name)["wet3D"], fill, gm.gridtopology.kind)
    return _phi[key]


def reference(oracle, name, which, rho="array", kap="grid", upwind=True):
    """The oracle's five matrices of a field (cached per (grid, field, ρ, κ, weighting); never modified by a test)."""
    key = (name, which, rho, kap, bool(upwind))
    if key not in _tm:
        g, gm = case(name)
        _tm[key] = oracle.transportmatrix(facefluxes(oracle, name, which), gm, indices(oracle, name), rho_of(name, rho), g.mlotst,
                                          *kappa(name, kap), upwind, tight=True)
    return _tm[key]


def rho_of(name, rho):
    return case(name)[0].rho if rho == "array" else RHO_SCALAR


# ---- facts about a grid that the CPU test asserts and the GPU tests rely on -------------------------------------------------------------------
def fill_tiles(N):
    return -(-N // TILE)


def scan_groups(ntiles):
    return -(-ntiles // SCAN_GROUP)


def tile_rows(name):
    """Per fill tile (256 consecutive wet ranks): how many (level, grid row) pairs its cells lie in, and whether it holds a cell of the last row
    (the tripolar seam: the heavy tiles otmb_tm_order deals over the XCDs)."""
    wet = wet_mask(name)
    nx, ny, nz = wet.shape
    L = np.flatnonzero(wet.ravel(order="F"))
    row = L // nx                       # (level * ny + j): a row of one level
    tile = np.arange(L.size) // TILE
    nt = fill_tiles(L.size)
    first = np.r_[True, (row[1:] != row[:-1]) | (tile[1:] != tile[:-1])]
    rows = np.bincount(tile[first], minlength=nt)
    seam = np.bincount(tile[(row % ny) == ny - 1], minlength=nt) > 0
    return rows, seam


def union_colptr(tm):
    """Column lengths of the union pattern."""
    N = len(tm["T"][0]) - 1
    keys = []
    for m in MATS[1:]:
        cp, rv, _ = tm[m]
        cols = np.repeat(np.arange(N, dtype=np.int64), np.diff(cp))
        keys.append(cols * (1 << 32) + rv)
    u = np.unique(np.concatenate(keys))
    return np.bincount(u >> 32, minlength=N)


def union_nnz(tm):
    """Entries of the union pattern of the four operators (T's reserved pattern)."""
    return int(union_colptr(tm).sum())


# ---- the synthetic sparse() call ----------------------------------------------------------------------------------------------------------------
SP_M, SP_N, SP_LEN = 4096, 700, 600000
SP_TILE, SP_GROUP = 256, 256 * 1024   # sorted entries per sp_heads tile, per scan group
SP_RUN, SP_BEFORE = 300, 40


def sparse_triplets():
    """(I, J, V, facts) for sparse(I, J, V, 4096, 700) with 600 000 triplets in random emission order.  In the order sparse() sorts them (by
    column, then row; stable):
      - one key holds a run of 300 duplicates that starts 40 entries before sorted position 262 144: it crosses the end of a 256-entry tile and
        the end of the first scan group of 1024 tiles;
      - another key's head sits exactly on a multiple of 256;
      - every eleventh value is 0.0 and one key's two values sum to exactly 0.0 (a stored zero is kept);
      - one key has the single value -0.0 (the first touch copies).
    facts: the four keys ((column - 1) * m + row - 1); check_sparse_triplets() verifies the placement from a stable argsort."""
    rng = np.random.default_rng([SEED, 3])
    m, n, ln = SP_M, SP_N, SP_LEN
    start = SP_GROUP - SP_BEFORE
    run_key = int(round(start / ln * m * n))
    below = np.sort(rng.integers(0, run_key, start))
    above = np.sort(rng.integers(run_key + 1, m * n, ln - start - SP_RUN))
    ks = np.concatenate([below, np.full(SP_RUN, run_key), above]).astype(np.int64)
    heads = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    length = np.diff(np.r_[heads, ln])
    aligned = heads[(heads % SP_TILE == 0) & (heads > start + SP_RUN)]
    pairs = heads[(length == 2) & (heads > start + SP_RUN)]
    singles = heads[(length == 1) & (heads > start + SP_RUN)]
    assert aligned.size and pairs.size and singles.size
    perm = rng.permutation(ln)
    key = np.empty(ln, np.int64)
    key[perm] = ks                                      # sorted position q is emitted at perm[q]
    V = rng.standard_normal(ln)
    V[::11] = 0.0
    zp, sp = int(pairs[len(pairs) // 2]), int(singles[len(singles) // 3])
    V[perm[zp]], V[perm[zp + 1]] = 2.5, -2.5
    V[perm[sp]] = -0.0
    facts = dict(run_key=run_key, aligned_key=int(ks[aligned[0]]), zero_key=int(ks[zp]), neg_key=int(ks[sp]))
    return key % m + 1, key // m + 1, V, facts


def check_sparse_triplets(I, J, V, facts):
    """The placement sparse_triplets() promises, from a stable argsort of the triplets as they are handed over."""
    key = (J - 1) * SP_M + (I - 1)
    assert I.size == SP_LEN and I.min() >= 1 and I.max() <= SP_M and J.min() >= 1 and J.max() <= SP_N
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], V[order]
    run = np.flatnonzero(ks == facts["run_key"])
    assert run.size == SP_RUN and run[0] == SP_GROUP - SP_BEFORE and run[-1] == run[0] + SP_RUN - 1
    assert run[0] // SP_TILE != run[-1] // SP_TILE and run[0] // SP_GROUP == 0 and run[-1] // SP_GROUP == 1
    assert np.count_nonzero(vs[run]) > SP_RUN // 2     # (real values to add across the boundary)
    al = np.flatnonzero(ks == facts["aligned_key"])
    assert al[0] % SP_TILE == 0 and al[0] > 0 and ks[al[0] - 1] != ks[al[0]]
    z = vs[ks == facts["zero_key"]]
    assert z.size == 2 and z[0] + z[1] == 0.0 and z[0] != 0.0
    s = vs[ks == facts["neg_key"]]
    assert s.size == 1 and s[0] == 0.0 and np.signbit(s[0])
    assert np.count_nonzero(V[::11]) <= 3               # every eleventh value is 0.0 (but for the few set above)
