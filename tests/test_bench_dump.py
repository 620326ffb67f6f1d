"""bench.py --dump-outputs: the result of the last timed step as DIR/<key>.npy (float32 / float64, at most 64 MB, a seeded pixel
sample beyond that), and --steps / ms_per_step as the line reports them.  The CPU tests feed dump_outputs a synthetic result dict;
the GPU test runs the benchmark on a small view twice and compares the dumps."""
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("iron_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _result(h, w, n_edge=5):
    g = torch.Generator().manual_seed(3)
    return {"convergent_mask": torch.rand(h, w, generator=g) > 0.5, "depth": torch.rand(h, w, generator=g),
            "color": torch.rand(h, w, 3, generator=g), "uv": torch.rand(h * w, 2, generator=g).double(),
            "edge_idx": [torch.arange(n_edge), torch.arange(n_edge)], "n_hits": 7}


def test_dump_writes_every_tensor_whole_under_the_budget():
    b = _bench()
    res = _result(16, 12)
    with tempfile.TemporaryDirectory() as d:
        info = b.dump_outputs(res, d)
        assert sorted(os.listdir(d)) == ["color.npy", "convergent_mask.npy", "depth.npy", "edge_idx.npy", "uv.npy"]
        assert info["sampled_pixels"] is None
        np.testing.assert_array_equal(np.load(os.path.join(d, "color.npy")), res["color"].numpy())
        m = np.load(os.path.join(d, "convergent_mask.npy"))
        assert m.dtype == np.float32 and np.array_equal(m, res["convergent_mask"].numpy().astype(np.float32))
        assert np.load(os.path.join(d, "uv.npy")).dtype == np.float64
        e = np.load(os.path.join(d, "edge_idx.npy"))
        assert e.dtype == np.float64 and e.shape == (10,)


def test_dump_samples_the_same_pixels_when_over_the_budget(monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_BYTES", 4000)
    res = _result(16, 12)
    with tempfile.TemporaryDirectory() as d1, tempfile.TemporaryDirectory() as d2:
        info = b.dump_outputs(res, d1)
        b.dump_outputs(res, d2)
        assert 0 < info["sampled_pixels"] < 16 * 12 and info["bytes"] <= 4000
        total = 0
        for name in os.listdir(d1):
            x1, x2 = np.load(os.path.join(d1, name)), np.load(os.path.join(d2, name))
            np.testing.assert_array_equal(x1, x2)
            total += x1.nbytes
        assert total == info["bytes"]
        depth = np.load(os.path.join(d1, "depth.npy"))
        color = np.load(os.path.join(d1, "color.npy"))
        assert depth.shape == (info["sampled_pixels"],) and color.shape == (info["sampled_pixels"], 3)
        # one sample for every per-pixel array: the depth and colour rows belong to the same pixels
        flat_d, flat_c = res["depth"].reshape(-1).numpy(), res["color"].reshape(-1, 3).numpy()
        idx = [int(np.flatnonzero(flat_d == v)[0]) for v in depth]
        assert idx == sorted(idx)
        np.testing.assert_array_equal(flat_c[idx], color)
        assert np.load(os.path.join(d1, "uv.npy")).shape == (16 * 12, 2)   # not on the pixel grid's shape: whole


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_repeat():
    """Two runs with the same arguments: the line reports the steps asked for and ms_per_step, and the dumps agree."""
    dumps = []
    with tempfile.TemporaryDirectory() as d:
        for run in range(2):
            out = os.path.join(d, "run%d" % run)
            r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--res", "128", "--no-extras",
                                "--no-cpu-baseline", "--dump-outputs", out], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-3000:]
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            assert line["steps"] == 2 and line["ms_per_step"] > 0
            assert "timed region" in r.stderr and "for 2 steps" in r.stderr
            assert line["dump_outputs"]["sampled_pixels"] is None
            dumps.append({n: np.load(os.path.join(out, n)) for n in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == sorted(b) and "color.npy" in a and "convergent_mask.npy" in a
    assert a["color.npy"].shape == (128, 128, 3) and a["color.npy"].dtype == np.float32
    assert a["convergent_mask.npy"].sum() > 0
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
