"""GPU: bench.py as the command line runs it. A plain run times the steps, prints the headline
fields and writes the last step's outputs; --full adds the passes that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_plain_and_full_line(tmp_path, full):
    """cfg2 at 5,000 rows: --steps is the number of timed steps, value and ms_per_step agree, the
    dumped log p sums to the dumped [sum log p, count] pair the NLL of the line comes from. Plain:
    no roofline, no CPU baseline, no nested MAF line. --full (CPU baseline and nested line switched
    off to keep the test short): the event pass ran."""
    extra = ["--full", "--no-cpu", "--no-secondary"] if full else []
    line = _bench("--steps", "3", "--warmup", "1", "--batch", "5000", "--dump-outputs", str(tmp_path), *extra)
    assert line["steps"] == 3 and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "fp32" and line["metric"].startswith("log_prob samples/sec/GPU")
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] * 1e-3 / 5000 - 1) < 1e-9
    assert line["full"] is full and "maf_d63" not in line and line["cpu_baseline"] is None
    if full:
        assert line["roofline"]["launches"] > 0 and line["roofline"]["frac"] > 0
    else:
        assert line["roofline"] is None
    lp, sums = np.load(tmp_path / "log_prob.npy"), np.load(tmp_path / "log_prob_sums.npy")
    assert lp.dtype == np.float32 and lp.shape == (5000,) and sums.dtype == np.float64 and sums[1] == 5000
    # each fp32 log p is within 2^-24 relative of the value the float64 sum took
    assert abs(lp.astype(np.float64).sum() - sums[0]) <= 2.0 ** -24 * np.abs(lp.astype(np.float64)).sum()
    assert abs(-sums[0] / sums[1] - line["nll_f64"]) <= 1e-12 * abs(line["nll_f64"])


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["sample4k", "train5k"])
def test_dump_of_sampling_and_training_steps(tmp_path, config):
    """The other kinds of step write what they return: samples and log-dets; the loss and the
    stepped weights. All finite, float32 or float64."""
    line = _bench("--config", config, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert line["steps"] == 2 and line["roofline"] is None and line["cpu_baseline"] is None
    files = sorted(os.listdir(tmp_path))
    if config == "sample4k":
        assert files == ["log_det.npy", "samples.npy"]
        assert np.load(tmp_path / "samples.npy").shape == (4000, 2) and np.load(tmp_path / "log_det.npy").shape == (4000,)
    else:
        assert "loss.npy" in files and np.load(tmp_path / "loss.npy").shape == (1,)
        assert sum(f.startswith("param.") for f in files) > 8
    for f in files:
        a = np.load(tmp_path / f)
        # (the loss is read off the step's float64 [sum, count] pair)
        assert a.dtype == (np.float64 if f == "loss.npy" else np.float32) and np.isfinite(a).all(), f
