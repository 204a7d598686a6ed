"""bench.py's plain run, --full and --dump-outputs: a plain run prints the headline line only, --full
adds the measurements that take runs of their own, --dump-outputs writes the last timed step's
latents as float32 .npy, identical from run to run for the same arguments."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

# the smallest shape the 1.3B model runs at in a blink: 2 latent frames of 16x16, S = 128 tokens
SMALL = ["--gpus", "1", "--model", "1.3B", "--frames", "5", "--height", "128", "--width", "128"]


def _run(monkeypatch, capsys, *extra):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + SMALL + list(extra))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_outputs_whole_float32(tmp_path):
    t = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).to(torch.bfloat16)
    bench.dump_outputs(str(tmp_path / "d"), {"latents": t})
    a = np.load(tmp_path / "d" / "latents.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 4)
    assert np.array_equal(a, t.float().numpy())


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    """Past the size limit the file holds a fixed sample: the same elements on every call, within
    the limit over all files."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 100)
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(7, 33, generator=g), torch.randn(40, generator=g)
    bench.dump_outputs(str(tmp_path / "a"), {"x": x, "y": y})
    bench.dump_outputs(str(tmp_path / "b"), {"x": x, "y": y})
    xa, ya = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "y.npy")
    assert xa.shape == (50,) and xa.dtype == np.float32
    assert np.array_equal(ya, y.numpy())                      # fits its share: whole
    assert xa.nbytes + ya.nbytes <= 400
    assert np.array_equal(xa, np.load(tmp_path / "b" / "x.npy"))
    assert np.isin(xa, x.numpy()).all()


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_latents(tmp_path, monkeypatch, capsys):
    a = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b = _run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "b"))
    for r in (a, b):
        assert r["steps"] == 3 and r["unit"] == "steps/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] / 1000 - 1) < 1e-2
        assert r["roofline"] is None and "e2e" not in r and "cpu_baseline" not in r
    la, lb = np.load(tmp_path / "a" / "latents.npy"), np.load(tmp_path / "b" / "latents.npy")
    assert os.listdir(tmp_path / "a") == ["latents.npy"]
    assert la.dtype == np.float32 and la.shape == (1, 16, 2, 16, 16) and np.isfinite(la).all()
    assert np.array_equal(la, lb)
    # --steps sets the number of timed steps: one step fewer leaves other latents
    _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "c"))
    assert not np.array_equal(la, np.load(tmp_path / "c" / "latents.npy"))


@pytest.mark.gpu
def test_full_run_adds_the_roofline(monkeypatch, capsys):
    r = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full", "--no-e2e", "--no-cpu-baseline")
    assert r["roofline"]["launches"] > 0 and r["roofline"]["achieved"] > 0
    assert r["config"]["step_exec"] == "hipGraph replay"
