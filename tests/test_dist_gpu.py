"""GPU: the depth-slab path with the HIP backend.  Two ranks share the box's single GPU and talk over
gloo (RCCL needs one GPU per rank; the transport layer is the only difference -- see otmb_amd.dist.Comm),
and the concatenated result must equal the whole-grid oracle bit for bit."""
import pytest

from helpers import COUNTS_ON
from test_dist_cpu import DEEP_SLABS, check_against_whole_grid, extended_slabs, mixed_levels, run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,rho", [(1, "array"), (2, "array"), (3, "scalar")])
def test_hip_slabs_match_whole_grid_oracle(oracle, tmp_path, world, rho):
    case = (24, 18, 11, 33, rho, "tripolar")
    z = run_ranks(world, "hip", case, tmp_path)
    check_against_whole_grid(oracle, z, case)


def test_hip_slabs_async_pipeline(oracle, tmp_path):
    case = (24, 18, 11, 34, "array", "tripolar")
    z = run_ranks(3, "hip", case, tmp_path, async_mode=True)
    check_against_whole_grid(oracle, z, case)


@pytest.mark.parametrize("pieces,world,async_mode", [(2, 2, False), (5, 3, True), (18, 3, False)])
def test_hip_slabs_chain_in_row_bands(oracle, tmp_path, pieces, world, async_mode):
    """The facefluxes chain handed over in row bands (otmb_facefluxes_rows_dev per piece): bit-identical to the whole-grid oracle."""
    case = (24, 18, 11, 35, "array", "tripolar")
    z = run_ranks(world, "hip", case, tmp_path, async_mode=async_mode, pieces=pieces)
    check_against_whole_grid(oracle, z, case)


def _kernels(outdir, world):
    import json
    import os

    return [json.load(open(os.path.join(outdir, f"kernels_{r}.json"))) for r in range(world)]


@pytest.mark.parametrize("world,async_mode,case", [(1, True, (24, 18, 11, 37, "array", "tripolar")), (2, False, (70, 9, 12, 38, "array", "tripolar")),
                                                   (3, True, (24, 18, 11, 39, "scalar", "tripolar")), (4, True, (24, 18, 11, 40, "array", "bipolar"))])
def test_hip_slabs_count_in_facefluxes(oracle, tmp_path, world, async_mode, case):
    """otmb_facefluxes_slab_counts_dev: every slab's facefluxes kernel counts for its own transportmatrix -- halo levels as neighbours,
    wet ranks from the slab's base -- so no rank launches a counting pass or a push-mask kernel, and the matrices are the whole-grid
    oracle's bit for bit."""
    z = run_ranks(world, "hip", case, tmp_path, async_mode=async_mode, extra_env={"OTMB_TEST_KERNELS": "1"})
    check_against_whole_grid(oracle, z, case)
    for k in _kernels(tmp_path, world):
        assert k.get("facefluxes_kernel", 0) > 0 and (("tm_count_kernel" not in k and "push_mask_kernel" not in k) or not COUNTS_ON), k


def test_hip_slabs_count_in_facefluxes_centred_weighting(oracle, tmp_path):
    case = (24, 18, 11, 42, "array", "tripolar")
    z = run_ranks(3, "hip", case, tmp_path, async_mode=True, extra_env={"OTMB_TEST_KERNELS": "1", "OTMB_TEST_CENTRED": "1"})
    check_against_whole_grid(oracle, z, case, upwind=False)
    for k in _kernels(tmp_path, 3):
        assert "tm_count_kernel" not in k or not COUNTS_ON, k


def test_hip_slabs_without_counts_still_count_for_themselves(oracle, tmp_path):
    case = (24, 18, 11, 37, "array", "tripolar")
    z = run_ranks(2, "hip", case, tmp_path, async_mode=True, extra_env={"OTMB_TEST_KERNELS": "1", "OTMB_COUNT_IN_FF": "0"})
    check_against_whole_grid(oracle, z, case)
    for k in _kernels(tmp_path, 2):
        assert k.get("tm_count_kernel", 0) > 0, k


@pytest.mark.parametrize("pieces,rows", [(3, "4"), (3, "1")])
def test_hip_slabs_count_in_row_bands(oracle, tmp_path, pieces, rows):
    """The chain in row bands: under the four-row wave geometry (large planes; forced here) every band adds its counts to the same
    buffer; under the one-row geometry a band is not a whole number of wave segments and the slab counts for itself."""
    case = (70, 9, 12, 41, "array", "tripolar")
    z = run_ranks(3, "hip", case, tmp_path, async_mode=True, pieces=pieces, extra_env={"OTMB_TEST_KERNELS": "1", "OTMB_FF_ROWS": rows})
    check_against_whole_grid(oracle, z, case)
    for k in _kernels(tmp_path, 3):
        assert ("tm_count_kernel" not in k) == (rows == "4" and COUNTS_ON), k


def _deep_slab_run(oracle, tmp_path, case, world, async_mode=False, upwind=True):
    """A run with the mixed layer five times as deep (its edge then passes level 64 of a 130-level grid): bit for bit the whole-grid
    oracle's matrices, and a rank counts in facefluxes exactly if its extended local grid -- from the partition the run used -- has at
    most 128 levels (FFC_MAX_NZ, otmb_facefluxes_slab_counts_dev); the others fall back to the plain kernel and count for themselves."""
    env = {"OTMB_TEST_KERNELS": "1", "OTMB_TEST_ML_SCALE": "5"}
    if not upwind:
        env["OTMB_TEST_CENTRED"] = "1"
    z = run_ranks(world, "hip", case, tmp_path, async_mode=async_mode, extra_env=env)
    idx, ref = check_against_whole_grid(oracle, z, case, upwind=upwind, ml_scale=5)
    assert mixed_levels(idx, ref, case[0] * case[1]).max() >= 65
    ext = extended_slabs(case, world)
    for n, k in zip(ext, _kernels(tmp_path, world)):
        assert k.get("facefluxes_kernel", 0) > 0, k
        assert ("tm_count_kernel" not in k) == (n <= 128 and COUNTS_ON), (ext, k)
    return ext


def _wet_beyond_local_level_64(case, world):
    """Per rank: wet owned cells on the levels that its counting kernel keeps in the upper registers (owned level 64 and deeper)."""
    from otmb_amd import dist as od, synthetic

    nx, ny, nz, seed, _, topo = case
    counts = synthetic.level_wet_counts(nx, ny, nz, seed=seed, topology=topo)
    return [int(counts[k0 + 64:k1].sum()) for k0, k1 in od.balanced_partition(counts, world)]


@pytest.mark.parametrize("world,async_mode,upwind", [(2, False, True), (3, True, True), (2, True, False)],
                         ids=["world2-sync", "world3-async", "world2-async-centred"])
def test_hip_slabs_count_on_more_than_64_local_levels(oracle, tmp_path, world, async_mode, upwind):
    """130 levels: some rank's extended slab has between 65 and 128 levels -- the upper registers of the per-level tables, the halo
    shift of the level index and of zt across the register boundary -- under both protocols, and once with centred weighting.  In two
    slabs the deeper one has water on its owned levels 64 and deeper and the mixed layer's edge among them; in three its last levels
    are dry (the grid's deepest water is near level 125), which leaves the clamps and the set-up of the upper registers."""
    ext = _deep_slab_run(oracle, tmp_path, DEEP_SLABS, world, async_mode, upwind)
    assert any(65 <= n <= 128 for n in ext) and all(n <= 128 for n in ext), ext
    if world == 2:
        assert _wet_beyond_local_level_64(DEEP_SLABS, 2)[1] > 0


def test_hip_one_rank_of_130_levels_counts_for_itself(oracle, tmp_path):
    ext = _deep_slab_run(oracle, tmp_path, DEEP_SLABS, 1, True)
    assert ext == [130]


def test_hip_slabs_deeper_slab_past_the_limit_falls_back(oracle, tmp_path):
    """200 levels in two slabs: the deeper one exceeds 128 extended levels and counts for itself, the upper one (more than 64) counts in
    facefluxes."""
    case = DEEP_SLABS[:2] + (200,) + DEEP_SLABS[3:]
    ext = _deep_slab_run(oracle, tmp_path, case, 2)
    assert 65 <= ext[0] <= 128 < ext[1], ext
    assert _wet_beyond_local_level_64(case, 2)[0] > 0


def _gpus():
    import torch

    return torch.cuda.device_count()  # (does not initialise the GPU in this process)


@pytest.mark.parametrize("async_mode", [False, True])
def test_hip_slabs_over_rccl_one_gpu_per_rank(oracle, tmp_path, async_mode):
    """BASELINE.json configs[3] in small, as it runs on a multi-GPU node: every rank its own GPU, the facefluxes chain's planes
    and the setup halos over RCCL (backend "nccl") point-to-point -- skipped on a one-GPU box.  Strong-scaled small grid,
    compared with the whole-grid oracle bit for bit."""
    n = _gpus()
    if n < 2:
        pytest.skip(f"needs at least 2 GPUs for one rank per GPU over RCCL ({n} visible)")
    world = min(n, 4)
    case = (24, 18, 12, 36, "array", "tripolar")
    z = run_ranks(world, "hip", case, tmp_path, async_mode=async_mode, rccl=True, timeout=600)
    check_against_whole_grid(oracle, z, case)
