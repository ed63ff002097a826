"""bench.py's plain run, --full and --dump-outputs: the plain result line holds the headline
figures and nothing that needs a measurement of its own, --steps sets the number of timed PPO
iterations, and the dumped outputs of two runs with the same arguments (one plain, one --full)
are identical array for array.  The benchmark runs in this process at 64 envs."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import bench

ENVS, T, STEPS = 64, 24, 2
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(monkeypatch, capsys, extra):
    # --no-gemm-table: the TunableOp switch is process-wide and would outlive this test
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                                      "--envs", str(ENVS), "--no-gemm-table"] + extra)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    with torch.random.fork_rng(devices=[0]):  # bench.main() seeds torch and numpy: leave no trace
        state = np.random.get_state()
        try:
            bench.main()
        finally:
            np.random.set_state(state)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_sample_to_budget_is_fixed_and_fits():
    rng = np.random.default_rng(0)
    arrays = {"big": rng.standard_normal((300, 100)).astype(np.float32),
              "bigger": rng.standard_normal(50000).astype(np.float32),
              "small": np.arange(10, dtype=np.float32)}
    whole = bench.sample_to_budget(arrays, budget=10 ** 6, small=1000)
    assert all(whole[k] is arrays[k] for k in arrays)
    cut = bench.sample_to_budget(arrays, budget=100000, small=1000)
    assert sum(a.nbytes for a in cut.values()) <= 100000
    assert cut["small"] is arrays["small"]
    assert cut["big"].size == int(30000 * (100000 - 40) / 320000) and cut["bigger"].size > cut["big"].size
    assert set(cut["big"].tolist()) <= set(arrays["big"].reshape(-1).tolist())
    again = bench.sample_to_budget(arrays, budget=100000, small=1000)
    assert all(np.array_equal(cut[k], again[k]) for k in arrays)


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path, monkeypatch, capsys):
    plain = _bench(monkeypatch, capsys, ["--dump-outputs", str(tmp_path / "plain")])
    for k in HEADLINE:
        assert k in plain, k
    assert plain["steps"] == STEPS and plain["unit"] == "env-steps/s" and plain["higher_is_better"] is True
    # value and ms_per_step describe the same timed region of STEPS iterations
    assert plain["value"] * plain["ms_per_step"] * 1e-3 == pytest.approx(ENVS * T, rel=1e-3)
    for k in ("roofline", "comm", "cpu_baseline"):
        assert k not in plain, k

    full = _bench(monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for k in HEADLINE:
        assert k in full, k
    assert full["metric"] == plain["metric"] and full["dtype"] == plain["dtype"]
    # one K_step launch in 4 of the timed region is bracketed: STEPS iterations of T env steps
    assert full["roofline"]["launches"] == STEPS * T // 4
    assert full["roofline"]["avg_launch_ms"] > 0 and "cpu_baseline" not in full

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    shapes = {"obs.npy": (ENVS, 705), "privileged_obs.npy": (ENVS, 219), "dof_pos.npy": (ENVS, 12),
              "rollout_actions.npy": (T, ENVS, 12), "rollout_returns.npy": (T, ENVS, 1), "losses.npy": (3,)}
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        assert n not in shapes or a.shape == shapes[n], (n, a.shape)
        np.testing.assert_array_equal(a, b, err_msg=n)
        total += a.nbytes
    assert set(shapes) <= set(names) and "policy_params.npy" in names
    assert total <= 64 * 2 ** 20
    # the dump is of a rollout that ran: the sampled actions are not one constant
    assert np.load(tmp_path / "plain" / "rollout_actions.npy").std() > 0
