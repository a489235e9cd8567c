"""bench.py's plain run and its --dump-outputs files: the dump is bounded, float32 and the same from run to run
(a fixed seeded row sample of an array over its share), a plain run carries no CPU baseline (--full adds it),
and the dumped arrays are what the library returns for the same inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("dmx_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_is_bounded_float32_and_repeatable(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)   # 2000 B a file: 166 rows of 3 float32
    big = np.arange(1000 * 3, dtype=np.float64).reshape(1000, 3)
    small = np.linspace(0.0, 1.0, 70, dtype=np.float32).reshape(10, 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("big", "small")}
    b = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in ("big", "small")}
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["big.npy", "small.npy"]
    assert a["big"].dtype == np.float32 and a["small"].dtype == np.float32
    assert np.array_equal(a["small"], small)
    assert a["big"].shape == (166, 3) and a["big"].nbytes + a["small"].nbytes <= 4000
    # whole rows of the input, in ascending row order, the same rows on both runs
    rows = (a["big"][:, 0] / 3).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["big"], big[rows].astype(np.float32))
    assert np.array_equal(a["big"], b["big"]) and np.array_equal(a["small"], b["small"])


def test_bench_options_exist():
    out = subprocess.run([sys.executable, BENCH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, timeout=60)
    assert out.returncode == 0, out.stdout
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in out.stdout, opt


@pytest.mark.gpu
def test_plain_run_dumps_what_the_library_returns(ctx, tmp_path):
    import depthmapx_amd as dmx
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--grid", "32",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "cells/s" and rec["dtype"] == "f64"
    assert rec["higher_is_better"] is True and rec["ms_per_step"] > 0
    assert abs(rec["value"] - rec["config"]["filled_cells"] / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert "cpu_baseline" not in rec and "vs_cpu_baseline" not in rec
    assert sorted(os.listdir(str(out))) == ["makegraph_attrs.npy", "vga_global.npy"]
    # the same inputs through the library
    bench = _bench_module()
    pm = dmx.PointMap([0.0, 0.0, 32.0, 32.0], bench.load_lines(32, 50), 1.0)
    assert pm.make_points(0.5, 0.5)
    g = pm.make_graph(ctx)
    vga, attrs = np.load(str(out / "vga_global.npy")), np.load(str(out / "makegraph_attrs.npy"))
    assert vga.dtype == np.float32 and attrs.dtype == np.float32
    assert vga.shape == (rec["config"]["filled_cells"], 7)
    assert np.array_equal(attrs.view(np.uint32), g.copy(runs=False)["attrs"].view(np.uint32))
    # the project's contract: makeGraph floats bit for bit (above), VGA floats within 1e-6, node counts exact
    ref = g.vga_visual_global()
    assert np.allclose(vga, ref, rtol=1e-6, atol=1e-6) and np.array_equal(vga[:, 5], ref[:, 5])
