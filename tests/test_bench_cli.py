"""bench.py's multi-GPU contract on the CPU: `--gpus N` is honoured with and
without a launcher.  --rehearse runs the rank plumbing
only (gloo process group, barrier-bracketed timing, max over ranks, rank 0's
single JSON line) -- the GPU path is exercised by the driver's runs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    env.update(kw)
    return env


def _run(args, env, timeout=240):
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_without_launcher_spawns_n_ranks(n):
    p = _run(["--gpus", str(n), "--rehearse", "--steps", "4", "--warmup", "0", "--dist-backend", "gloo"], _env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == n and rec["ranks_timed"] == n and rec["rehearsal"] is True


@pytest.mark.timeout(120)
def test_launcher_world_size_must_match_gpus():
    p = _run(["--gpus", "2", "--rehearse"], _env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert p.returncode != 0
    assert "WORLD_SIZE=1" in p.stderr


@pytest.mark.timeout(120)
def test_one_gpu_rehearsal_single_rank():
    p = _run(["--rehearse", "--steps", "2"], _env())
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 1


@pytest.mark.timeout(300)
def test_under_torch_distributed_run():
    """The driver's launcher form: torch.distributed.run with --nproc-per-node N and --gpus N."""
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29613", BENCH, "--gpus", "2", "--rehearse",
                        "--steps", "3"], env=_env(), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(recs) == 1 and recs[0]["n_gpus"] == 2


def test_resolution_override():
    """--resolution keeps the config's world, flags and GI schedule and changes only the frame size
    (odd sizes included); the metric's description names the new size."""
    import importlib
    import sys as _sys
    _sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    from rvgrt_amd.configs import CONFIGS
    c = bench.bench_config("c4", "1707x961")
    base = CONFIGS["c4"]
    assert (c.width, c.height) == (1707, 961)
    assert (c.log2_n, c.flags, c.gi_sweeps, c.gi_per_frame) == (base.log2_n, base.flags, base.gi_sweeps, base.gi_per_frame)
    assert "1707x961" in c.describe and "3840x2160" not in c.describe
    assert bench.bench_config("c3") is CONFIGS["c3"]
    with pytest.raises(SystemExit):
        bench.bench_config("c3", "1x5")


def test_world_override():
    import importlib
    import sys as _sys
    _sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    c = bench.bench_config("c4", world=9)
    assert c.log2_n == 9 and c.n == 512 and "512^3" in c.describe and "1024^3" not in c.describe
    c = bench.bench_config("c4", "1280x720", 11)
    assert (c.width, c.height, c.n) == (1280, 720, 2048)
    with pytest.raises(SystemExit):
        bench.bench_config("c4", world=12)


def _bench():
    import importlib
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def _frame_images(w, h, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return {"color": rng.integers(0, 256, (h, w, 4), dtype=np.uint8),
            "motion": rng.uniform(-2, 2, (h, w, 2)).astype(np.float16).view(np.uint16),
            "depth": rng.uniform(0, 1, (h, w)).astype(np.float16).view(np.uint16)}


def test_dump_outputs_small_frame_is_written_whole(tmp_path):
    """--dump-outputs: a frame inside the budget is written whole, float32, RGBA8 as 0..255 and the
    half-float images as their values."""
    import numpy as np
    bench = _bench()
    im = _frame_images(37, 21, 1)
    info = bench.dump_outputs(str(tmp_path / "o"), im)
    assert info["pixels"] == 37 * 21 and info["sample_seed"] is None
    got = {n: np.load(tmp_path / "o" / f"{n}.npy") for n in im}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["color"], im["color"].astype(np.float32))
    assert np.array_equal(got["motion"], im["motion"].view(np.float16).astype(np.float32))
    assert got["depth"].shape == (21, 37) and info["arrays"]["depth"] == {"shape": [21, 37], "non_finite": 0}


def test_dump_outputs_large_frame_is_a_fixed_sample(tmp_path):
    """A 4K frame exceeds the budget: every image keeps the same sorted, seeded pixel sample, the same from
    call to call, and the whole set stays under 64 MB."""
    import numpy as np
    bench = _bench()
    w, h = 3840, 2160
    im = _frame_images(w, h, 2)
    a = bench.dump_outputs(str(tmp_path / "a"), im)
    im2 = {k: v.copy() for k, v in im.items()}
    im2["color"][::7, ::5] ^= 1          # another build's frame: the sample must not depend on the data
    b = bench.dump_outputs(str(tmp_path / "b"), im2)
    assert a["pixels"] == b["pixels"] == bench.DUMP_BUDGET_BYTES // 28 < w * h and a["sample_seed"] == 0
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
    idx = np.sort(np.random.default_rng(0).choice(w * h, size=a["pixels"], replace=False))
    for n in im:
        ga, gb = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert ga.dtype == np.float32 and ga.shape[0] == a["pixels"]
        src = im[n].view(np.float16) if im[n].dtype == np.uint16 else im[n]
        assert np.array_equal(ga, src.reshape((w * h,) + src.shape[2:])[idx].astype(np.float32))
        src2 = im2[n].view(np.float16) if im2[n].dtype == np.uint16 else im2[n]
        assert np.array_equal(gb, src2.reshape((w * h,) + src2.shape[2:])[idx].astype(np.float32))


def test_plain_and_full_options(tmp_path):
    """--full and --dump-outputs exist, and --steps 0 is refused (it must set the number of timed steps)."""
    p = _run(["--help"], _env())
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = _run(["--rehearse", "--steps", "0"], _env())
    assert p.returncode == 2 and "--steps" in p.stderr
    p = _run(["--rehearse", "--steps", "3", "--full", "--dump-outputs", str(tmp_path / "d")], _env())
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["steps"] == 3


def test_recorded_bench_line_keeps_the_contract():
    """The --full bench line, as last recorded on the GPU (profiles/r06/final/driver_bench.json):
    every contract key, the roofline object (algorithmic bytes / launch time against the 8 TB/s peak,
    with the PMC traffic) and the CPU baseline object."""
    path = os.path.join(ROOT, "profiles", "r06", "final", "driver_bench.json")
    d = json.loads(open(path).read().strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["config"]["workload"] == "c4" and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    # achieved = algorithmic bytes per launch / the measured launch time
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["avg_launch_ms"] * 1e-3) / 1e9) < 0.01 * rf["achieved"]
    assert rf["traffic"] and rf["traffic"] > 0
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] >= 1
    # value = rays per frame x frames per second
    assert abs(d["value"] - d["rays_per_frame"] / (d["ms_per_step"] * 1e-3) / 1e6) < 0.01 * d["value"]
