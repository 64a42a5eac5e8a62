"""Guards the driver contract: bench.py must emit ONE JSON line with
the agreed schema, on CPU and under torchrun-style env."""

import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


def run_bench(extra, env_extra=None):
    env = dict(os.environ)
    if env_extra:
        env.update(env_extra)
    r = subprocess.run(
        [sys.executable, os.path.join(HERE, "bench.py"), "--steps", "2",
         "--warmup", "1", "--batch-size", "4", "--image-size", "32"] + extra,
        capture_output=True, text=True, timeout=600, env=env, cwd=HERE)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().splitlines()
             if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def check_schema(d, n_gpus=1):
    for k in REQUIRED:
        assert k in d, k
    assert d["metric"] == "samples/sec (whole node)"
    assert d["n_gpus"] == n_gpus
    assert d["value"] > 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["dtype"] in ("bf16", "fp32")
    assert "model" in d["config"] and "global_batch" in d["config"]
    assert "parallelism" in d["config"]


def test_bench_default_cpu():
    d = run_bench([])
    check_schema(d)
    assert d["config"]["parallelism"] == "dp1"


def test_bench_hips_flags_cpu():
    d = run_bench(["--mode", "hips", "--compress", "fp16",
                   "--wan-gbps", "10"])
    check_schema(d)  # single process -> falls back to dp1 topology


def test_bench_full_flag_cpu():
    # --full adds measurements around the headline figure; the result
    # line keeps its schema and meaning
    d = run_bench(["--full"])
    check_schema(d)
    assert d["steps"] == 2 and d["warmup"] == 1


def test_bench_dump_outputs_cpu(tmp_path):
    import numpy as np
    dumps = []
    for sub in ("a", "b"):
        out = tmp_path / sub
        check_schema(run_bench(["--dump-outputs", str(out)]))
        files = sorted(p.name for p in out.iterdir())
        assert "loss.npy" in files and "logits.npy" in files
        assert any(f.startswith("param.") for f in files)
        assert sum(p.stat().st_size for p in out.iterdir()) <= 64 << 20
        dumps.append({f: np.load(out / f) for f in files})
    a, b = dumps
    assert a.keys() == b.keys()
    assert a["logits.npy"].shape == (4, 10)
    for f in a:
        assert a[f].dtype == np.float32
        assert np.isfinite(a[f]).all()
        # same arguments -> same inputs -> same outputs (fp32 on CPU,
        # up to reduction order)
        np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=1e-6)


def test_bench_dump_outputs_samples_large_arrays(tmp_path, monkeypatch):
    import numpy as np
    import torch
    # importing bench sets a MIOpen default in the environment: undo it
    # after this test so the rest of the session is unaffected
    monkeypatch.setenv("MIOPEN_FIND_MODE",
                       os.environ.get("MIOPEN_FIND_MODE", "1"))
    import bench
    big = torch.arange(bench.DUMP_ARRAY_ELEMS + 7, dtype=torch.float32)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub),
                           {"small": torch.ones(3, 5), "big": big})
    a = np.load(tmp_path / "a" / "big.npy")
    assert a.shape == (bench.DUMP_ARRAY_ELEMS,)
    assert np.array_equal(a, np.load(tmp_path / "b" / "big.npy"))
    assert np.load(tmp_path / "a" / "small.npy").shape == (3, 5)


def test_bench_value_consistency():
    d = run_bench([])
    # value == n_gpus * per_gpu_batch * 1000 / ms_per_step
    expect = d["n_gpus"] * d["config"]["per_gpu_batch"] * 1e3 / d["ms_per_step"]
    assert abs(expect - d["value"]) / expect < 0.01
