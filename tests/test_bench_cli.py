"""bench.py's command line: a plain run measures the headline only, ``--full`` turns every secondary
measurement on, ``--dump-outputs`` writes the last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("frozen", "small_batch", "diag", "measured_peaks", "cpu_baseline", "roofline_dw", "roofline_wgrad")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_every_secondary_measurement_off(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.mode) == (7, 2, "unfrozen")
    assert (a.cpu_baseline, a.measured_peaks, a.diag, a.small_batch, a.kernel_timing) == ("off", "off", "off", 0, False)
    assert not a.full and a.dump_outputs is None


def test_full_run_has_them_on_and_single_options_still_work(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.mode == "both"
    assert (a.cpu_baseline, a.measured_peaks, a.diag, a.small_batch, a.kernel_timing) == ("on", "on", "on", 4, True)
    a = _parse(monkeypatch, "--full", "--cpu-baseline", "off", "--small-batch", "0", "--no-kernel-timing",
               "--mode", "frozen")
    assert (a.cpu_baseline, a.measured_peaks, a.small_batch, a.kernel_timing, a.mode) == ("off", "on", 0, False, "frozen")
    a = _parse(monkeypatch, "--diag", "on")
    assert (a.diag, a.cpu_baseline, a.mode) == ("on", "off", "unfrozen")
    assert _parse(monkeypatch, "--model", "lstma", "--full").mode == "frozen"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    """A plain run at a small shape (2 clips x 4 frames x 96^2): one JSON line with the headline keys,
    --steps timed steps, none of the --full keys; --dump-outputs leaves finite float32 / float64 arrays
    of the documented names and shapes, under 64 MB."""
    B, T, S, steps = 2, 4, 96, 3
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(B), "--frames", str(T), "--size", str(S), "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["unit"] == "clips/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 / B - 1) < 1e-3
    assert out["roofline"] is None and not [k for k in EXTRAS if k in out]
    arrays = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert set(arrays) == {"loss", "output", "features", "grads_sample", "params_sample", "grads_norms", "params_norms"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["output"].shape == (B, 1) and arrays["features"].shape == (B, T, 2048)
    assert arrays["grads_sample"].shape == arrays["params_sample"].shape
    assert arrays["grads_norms"].shape == arrays["params_norms"].shape and (arrays["grads_norms"] > 0).any()
    assert abs(float(arrays["loss"].reshape(-1)[0]) - out["loss"]) < 1e-4
