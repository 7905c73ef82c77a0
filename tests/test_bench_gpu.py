"""GPU: bench.py itself, as the driver starts it (run with -m gpu).  (1) `python bench.py` on the small workload prints exactly one JSON
line with the contract's keys, a live roofline record and the product library's kernels; (2) the launcher form -- `python -m
torch.distributed.run --nproc-per-node 1 ... bench.py --gpus 1` with OTMB_FORCE_SLAB=1 -- takes the depth-slab path with ONE rank over
the "nccl" backend (= RCCL): communicator bring-up with device_id, barrier and the max-over-ranks all_reduce of the timing on this image
and this GPU.  A box with one GPU cannot run two RCCL ranks (tests/test_dist_gpu.py skips those); this is the part of that path it can run."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--workload", "small", "--steps", "3", "--warmup", "1", "--repeats", "2", "--no-cpu-baseline", "--no-end-to-end", "--extra-configs=", "--full"]
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
            "roofline")


def _one_json_line(r):
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "OTMB_FORCE_SLAB")}
    env.update(extra)
    return env


def test_bench_prints_one_contract_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *COMMON], env=_clean_env(), capture_output=True, text=True, timeout=600)
    d = _one_json_line(r)
    for k in CONTRACT:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "wet-cells/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and "synthetic" in d["data"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["wet_cells"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    # the kernels of the product library ran (HIP events on the launch stream), the fill pass among them
    assert d["kernels_ms"]["tm_kernel<fill>"] > 0 and d["kernels_ms"]["facefluxes_kernel"] > 0


def test_bench_as_one_rank_over_rccl():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "1", *COMMON]
    r = subprocess.run(cmd, env=_clean_env(OTMB_FORCE_SLAB="1", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=900)
    d = _one_json_line(r)
    assert d["n_gpus"] == 1 and d["unit"] == "wet-cells/s" and d["value"] > 0
    assert d["config"].get("ranks_over") == "nccl", d["config"]  # the depth-slab path, its rank over RCCL
    assert d["roofline"] is not None and 0 < d["roofline"]["frac"] < 1


def test_plain_run_times_k_steps_and_dumps_the_last_steps_outputs(tmp_path, oracle):
    """Without --full the line carries the headline alone, over exactly K steps timed once; --dump-outputs writes the last step's matrices
    and face fluxes, which on the small grid (fewer cells than the sample) are the whole outputs -- the oracle's, bit for bit."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import otmb_amd
    from otmb_amd import synthetic

    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "small", "--steps", "4", "--warmup", "1", "--dump-outputs", str(out)],
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    d = _one_json_line(r)
    assert d["steps"] == 4 and d["repeats"]["n"] == 1 and d["full"] is False and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["roofline"] is None and d["kernels_ms"] == {}
    for k in ("fused_step", "given_ops_step", "end_to_end", "cpu_baseline", "config2", "box_probe", "config3", "config5"):
        assert k not in d, k
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) <= 64 << 20

    g = synthetic.make_grid(*synthetic.PRESETS["small"][:3], seed=d["config"]["seed"], land_fraction=synthetic.PRESETS["small"][3], rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    idx = oracle.makeindices(gm.v3D)
    phi = oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], g.umo.properties["_FillValue"], gm.gridtopology.kind)
    ref = oracle.transportmatrix(phi, gm, idx, g.rho, g.mlotst, g.kappaH, g.kappaVML, g.kappaVdeep, True)
    N = idx["N"]
    assert list(files["nnz.npy"]) == [N, *(len(ref[m][1]) for m in oracle.MATS)]
    assert np.array_equal(files["columns.npy"], np.arange(N))
    for m, name in zip(oracle.MATS, ("T", "Tadv", "TkH", "TkVML", "TkVdeep")):
        cp, rv, nz = ref[m]
        assert np.array_equal(files[name + "_colptr.npy"], np.stack([cp[:-1] - cp[0], cp[1:] - cp[0]], axis=1)), m
        assert np.array_equal(files[name + "_rowval.npy"], rv) and np.array_equal(files[name + "_nzval.npy"], nz), m
    assert np.array_equal(files["cells.npy"], np.arange(g.umo.data.size))
    for face in ("east", "west", "north", "south", "top", "bottom"):
        assert np.array_equal(files[f"phi_{face}.npy"], phi[face].ravel(order="F"), equal_nan=True), face
