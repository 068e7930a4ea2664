"""bench.py on the GPU at a small size: a plain run measures the headline
and nothing else, --full adds the rest, --steps sets the timed steps, and
--dump-outputs writes the same games for the same arguments (so two builds
can be compared array for array)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--slots", "256", "--sims", "16", "--steps", "6", "--warmup", "2", "--cache-log2", "14"]
FULL_ONLY = ("roofline_tree", "cache_off", "cpu_baseline", "cpu_baseline_native", "cpu_baseline_configs0")


def _run(extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + SMALL + extra, capture_output=True,
                       text=True, timeout=120, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_full_adds_the_rest_and_the_dumps_agree(tmp_path):
    plain = _run(["--dump-outputs", str(tmp_path / "plain")])
    full = _run(["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for line in (plain, full):
        assert line["steps"] == 6 and line["unit"] == "games/s" and line["higher_is_better"] is True
        assert line["value"] > 0 and line["ms_per_step"] > 0 and "Connect-4 6x7, 16 sims/move" in line["metric"]
        # the window's simulations: --steps moves of every slot
        assert round(line["simulations_per_s"] * line["ms_per_step"] * 1e-3 * 6) == pytest.approx(6 * 256 * 16, rel=1e-3)
        assert line["games_timed"] == line["dump_outputs"]["of"] == line["dump_outputs"]["games"] > 0
        assert line["roofline"]["launches_timed"] > 0  # the tower's events ride in the timed window itself
    assert plain["full"] is False and full["full"] is True
    assert all(plain[k] is None for k in FULL_ONLY) and "isolated" not in plain["roofline"]
    assert full["roofline_tree"]["avg_launch_ms"] > 0 and full["cache_off"]["value"] > 0
    assert full["roofline"]["isolated"]["avg_launch_ms"] > 0 and full["cpu_baseline"] is None
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) == sorted(
        k + ".npy" for k in ("game_ids", "lengths", "results", "expansions", "boards", "policies", "moves"))
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype in (np.float32, np.float64) and len(a) == plain["games_timed"], f
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f
        total += a.nbytes
    assert total == plain["dump_outputs"]["bytes"] <= 64 << 20
    lengths = np.load(tmp_path / "plain" / "lengths.npy").astype(int)
    pol = np.load(tmp_path / "plain" / "policies.npy")
    assert np.all(np.diff(np.load(tmp_path / "plain" / "game_ids.npy")) > 0) and lengths.min() >= 7
    for g, T in enumerate(lengths):  # every played ply carries a policy, nothing after it
        np.testing.assert_allclose(pol[g, :T].sum(-1), 1.0, atol=1e-12)
        assert not pol[g, T:].any()

