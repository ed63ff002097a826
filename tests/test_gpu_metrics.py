"""Gait metrics on the GPU: k_metrics_sample / k_metrics_fold (hg_metrics_sample, hg_metrics_fold,
hg_metrics_clear) against the float64 reference of tests/metrics_ref.py on the planted rows of
tests/metrics_cases.py and on a driven env; where env.step() puts the two calls; that the feature
off leaves nothing behind; the runner's gait_* statistics.

Bound on the float sums: relative 1e-12 with absolute 1e-15 (metrics_ref.RTOL / ATOL; the derivation
is in tests/test_metrics_cases.py), at most 100 accumulated steps; counters and the integer-valued
slots are compared exactly.  Env counts 1, 3 and 65 (np = 128: the second wave is partly filled).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import metrics_cases as MC
import metrics_ref as MR
from test_gpu_parity import _make_env, _need_gpu

pytestmark = pytest.mark.gpu

f32 = np.float32
VIEW_OF = {"root_states": "root_states", "commands": "commands", "torques": "torques", "dof_vel": "dof_vel",
           "contact_forces": "contact_forces", "rigid_state": "rigid_state", "actions": "actions",
           "last_actions": "last_actions"}


def _g(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _lib():
    from humanoid import _native as N
    return N, N.lib()


def _stream(env):
    return ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)


def _plant(env, state):
    """Planted state through the views (the arena's SoA regions behind them)."""
    for k, attr in VIEW_OF.items():
        getattr(env, attr).copy_(torch.from_numpy(state[k]).to(env.device))


def _read(env):
    """The eight arrays the sample reads, as the views show them, env-major float32 on the host."""
    torch.cuda.synchronize()
    return {k: getattr(env, attr).detach().cpu().numpy().copy() for k, attr in VIEW_OF.items()}


def _acc(env):
    return _g(env.metrics_running), _g(env.metrics_completed), _g(env.metrics_counts).astype(np.int64)


def _padded(env, tid, rows, dtype):
    """The whole [rows, np] buffer behind a metrics view, padding columns included."""
    N, L = _lib()
    d = N.HgDesc()
    N.check(L.hg_tensor(env.sim, N.T[tid], ctypes.byref(d)), env.sim)
    np_ = int(d.strides[0])
    es = torch.empty((), dtype=dtype).element_size()
    return _g(env._arena_base.view(dtype).as_strided([rows, np_], [np_, 1], d.offset_bytes // es))


def _planted_env(n):
    """An env of n with metrics on, its torque limits set to the table's, accumulators cleared."""
    N, L = _lib()
    env = _make_env(n, metrics__gait=True)
    for j in range(12):
        env._hgcfg.torque_limit[j] = float(MC.TORQUE_LIMIT[j])
    N.check(L.hg_update_cfg(env.sim, ctypes.byref(env._hgcfg), _stream(env)), env.sim)
    assert tuple(env._hgcfg.feet_body) == MC.FEET
    assert float(env._hgcfg.sim_dt) * int(env._hgcfg.decimation) == MC.DT
    env.clear_gait_metrics()
    return env


def _compare(label, got, want, worst):
    run, done, cnt = got
    rrun, rdone, rcnt = want
    np.testing.assert_array_equal(cnt, rcnt, err_msg=label)
    assert np.isfinite(run).all() and np.isfinite(done).all(), label
    for name, a, b in (("running", run, rrun), ("completed", done, rdone)):
        dev = MR.max_deviation(a, b)
        worst[0] = max(worst[0], dev)
        assert dev <= 1.0, f"{label}: {name} rows deviate {dev:.3e} x the bound"
        for s in ("steps", "double_support", "flight", "peak_torque"):
            np.testing.assert_array_equal(a[MR.NAMES.index(s)], b[MR.NAMES.index(s)], err_msg=f"{label} {name} {s}")


# ---------------------------------------------------------------- planted passes
@pytest.mark.parametrize("n", [1, 3, 65])
def test_sample_on_planted_rows(n):
    """hg_metrics_sample alone, round after round on the table's rows (env e sees row e + round * n),
    against the reference replay; skipped rows leave their running row's bits alone."""
    _need_gpu()
    N, L = _lib()
    env = _planted_env(n)
    R = len(MC.ROWS)
    rounds = min(-(-R // n) + 1, 100)
    run, cnt = np.zeros((13, n)), np.zeros((4, n), np.int64)
    worst = [0.0]
    for r in range(rounds):
        idx = [(e + r * n) % R for e in range(n)]
        st = MC.stack(idx)
        _plant(env, st)
        before = _g(env.metrics_running)
        assert L.hg_metrics_sample(env.sim, _stream(env)) == 0
        run, cnt = MR.sample(st, MC.TORQUE_LIMIT, MC.DT, run, cnt)
        got = _acc(env)
        skipped = np.array([MC.SKIPPED[i] for i in idx])
        assert np.array_equal(got[0][:, skipped], before[:, skipped])
        _compare(f"n={n} round {r}", got, (run, np.zeros((13, n)), cnt), worst)
    print(f"planted sample, n = {n}: {rounds} rounds, largest deviation {worst[0]:.3e} x the bound "
          f"(rtol {MR.RTOL}, atol {MR.ATOL}); skipped {cnt[3].sum()}")
    assert cnt[3].sum() > 0 and run[0].sum() > 0
    if n == 65:
        for tid, rows, dt in (("METRICS_RUN", 13, torch.float64), ("METRICS_DONE", 13, torch.float64),
                              ("METRICS_COUNT", 4, torch.int32)):
            full = _padded(env, tid, rows, dt)
            assert full.shape == (rows, 128) and not full[:, 65:].any(), tid


@pytest.mark.parametrize("n", [1, 3, 65])
def test_fold_on_planted_flags(n):
    """Fold mode 0 on planted reset / time-out patterns (none, all, a reset env with an empty running
    row, mixed) and fold mode 1 with a mask and with NULL, against the reference after every call."""
    _need_gpu()
    N, L = _lib()
    env = _planted_env(n)
    R = len(MC.ROWS)
    e = np.arange(n)
    ref = [np.zeros((13, n)), np.zeros((13, n)), np.zeros((4, n), np.int64)]
    worst = [0.0]
    shift = [0]

    def sample():
        idx = [(k + shift[0]) % R for k in range(n)]
        shift[0] += 1 if n > 1 else 4      # n = 1 walks walking, mixed_power, double_support, a NaN row, ...
        st = MC.stack(idx)
        _plant(env, st)
        assert L.hg_metrics_sample(env.sim, _stream(env)) == 0
        ref[0], ref[2] = MR.sample(st, MC.TORQUE_LIMIT, MC.DT, ref[0], ref[2])

    def fold0(reset, time_out, label):
        env._reset_u8.copy_(torch.from_numpy(reset.astype(np.uint8)).to(env.device))
        env._timeout_u8.copy_(torch.from_numpy(time_out.astype(np.uint8)).to(env.device))
        assert L.hg_metrics_fold(env.sim, 0, None, _stream(env)) == 0
        ref[:] = MR.fold(ref[0], ref[1], ref[2], 0, reset=reset, time_out=time_out)
        _compare(f"n={n} {label}", _acc(env), ref, worst)

    def fold1(mask, label):
        m = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).to(env.device)
        assert L.hg_metrics_fold(env.sim, 1, None if m is None else ctypes.c_void_p(m.data_ptr()), _stream(env)) == 0
        torch.cuda.synchronize()
        ref[:] = MR.fold(ref[0], ref[1], ref[2], 1, mask=mask)
        _compare(f"n={n} {label}", _acc(env), ref, worst)

    zeros, ones = np.zeros(n, bool), np.ones(n, bool)
    sample()
    fold0(zeros, e % 2 == 0, "no reset")                        # time-out flags alone end nothing
    assert ref[2][0].sum() == 0
    had = ref[0][0] > 0
    fold0(ones, e % 2 == 1, "all reset")                        # falls on even envs, time-outs on odd ones
    episodes = ref[2][0].copy()
    np.testing.assert_array_equal(episodes, had.astype(np.int64))
    fold0(ones, zeros, "all reset again, empty rows")           # steps == 0: not an episode
    np.testing.assert_array_equal(ref[2][0], episodes)
    sample()
    sample()
    fold0(e % 3 == 0, e % 2 == 0, "mixed")
    sample()
    fold1(e % 2 == 1 if n > 1 else ones, "discard masked")
    sample()
    before = [a.copy() for a in ref]
    fold1(None, "discard all")
    assert not ref[0].any() and np.array_equal(ref[1], before[1]) and np.array_equal(ref[2], before[2])
    sample()
    fold0(ones, ones, "all time out")
    c = ref[2]
    assert c[0].sum() > 0 and (c[1] + c[2] == c[0]).all()
    if n >= 3:
        assert c[1].sum() > 0 and c[2].sum() > 0
    print(f"planted fold, n = {n}: largest deviation {worst[0]:.3e} x the bound; episodes {c[0].sum()}, falls "
          f"{c[1].sum()}, time-outs {c[2].sum()}, skipped {c[3].sum()}")
    if n == 65:
        for tid, rows, dt in (("METRICS_RUN", 13, torch.float64), ("METRICS_DONE", 13, torch.float64),
                              ("METRICS_COUNT", 4, torch.int32)):
            assert not _padded(env, tid, rows, dt)[:, 65:].any(), tid
    # an unknown mode is refused before any launch, with a reason; clear zeroes all three
    assert L.hg_metrics_fold(env.sim, 2, None, _stream(env)) == 1
    assert b"mode" in L.hg_last_error(env.sim)
    _compare(f"n={n} after the refusal", _acc(env), ref, worst)
    env.clear_gait_metrics()
    assert not any(a.any() for a in _acc(env))


# ---------------------------------------------------------------- wiring
STEPS, TIMEOUT_AT, TIP_AT, RESET_AT = 40, 6, 3, 25


def _actions(k, n, device):
    g = torch.Generator().manual_seed(1000 + k)
    return (0.3 * torch.randn(n, 12, generator=g)).to(device)


def _intervene(env, k):
    """Before step k: env 1 is put one step from its time-out, env 2 is tipped onto its side just
    above the ground (its base box lands within a few steps: a fall)."""
    if k == TIMEOUT_AT:
        env.episode_length_buf[1] = int(env.max_episode_length)
    if k == TIP_AT:
        root = env.root_states[2].clone()
        root[2] = env.env_origins[2, 2] + 0.24
        root[3:7] = torch.tensor([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)], dtype=torch.float32)
        root[7:13] = 0.0
        env.root_states[2] = root


def test_wiring_manual_sequence_and_twin_step():
    """An env of 3 driven through the ABI (hg_step, read the views, hg_metrics_sample, hg_post,
    hg_metrics_fold) with a forced time-out, a forced fall and a reset_idx in the middle: the
    reference replayed from what was read gives the device's accumulators; a twin env with the same
    seed driven through env.step() / env.reset_idx() alone ends with the same bits."""
    _need_gpu()
    N, L = _lib()
    n = 3
    env = _make_env(n, metrics__gait=True)
    twin = _make_env(n, metrics__gait=True)
    lim = [float(env._hgcfg.torque_limit[j]) for j in range(12)]
    dt = float(env._hgcfg.sim_dt) * int(env._hgcfg.decimation)
    feet = tuple(env._hgcfg.feet_body)
    ref = [np.zeros((13, n)), np.zeros((13, n)), np.zeros((4, n), np.int64)]
    for a in _acc(env) + _acc(twin):      # creation's reset discarded, nothing counted
        assert not a.any()
    s = _stream(env)
    mask = torch.tensor([1, 0, 0], dtype=torch.uint8, device=env.device)
    for k in range(STEPS):
        act = _actions(k, n, env.device)
        for e_ in (env, twin):
            _intervene(e_, k)
        if k == RESET_AT:
            assert ref[0][0, 0] > 0       # env 0 is mid-episode: the reset discards these steps
            N.check(L.hg_reset_masked(env.sim, ctypes.c_void_p(mask.data_ptr()), ctypes.c_uint64(env.common_step_counter), s), env.sim)
            N.check(L.hg_metrics_fold(env.sim, 1, ctypes.c_void_p(mask.data_ptr()), s), env.sim)
            ref[:] = MR.fold(ref[0], ref[1], ref[2], 1, mask=[1, 0, 0])
            twin.reset_idx([0])
        # the manual sequence
        N.check(L.hg_step(env.sim, ctypes.c_void_p(act.data_ptr()), ctypes.c_uint64(env.common_step_counter), s), env.sim)
        env.common_step_counter += 1
        st = _read(env)
        N.check(L.hg_metrics_sample(env.sim, s), env.sim)
        N.check(L.hg_post(env.sim, ctypes.c_uint64(env.common_step_counter), s), env.sim)
        N.check(L.hg_metrics_fold(env.sim, 0, None, s), env.sim)
        reset, time_out = _g(env._reset_u8), _g(env._timeout_u8)
        ref[0], ref[2] = MR.sample(st, lim, dt, ref[0], ref[2], feet)
        ref[:] = MR.fold(ref[0], ref[1], ref[2], 0, reset=reset, time_out=time_out)
        # the twin: env.step() alone
        twin.step(act)
    got = _acc(env)
    worst = [0.0]
    _compare("wiring", got, ref, worst)
    c = got[2]
    print(f"wiring: {STEPS} steps, largest deviation {worst[0]:.3e} x the bound; episodes {c[0]}, falls {c[1]}, "
          f"time-outs {c[2]}, skipped {c[3]}")
    assert c[2][1] >= 1, "env 1 did not time out"
    assert c[1][2] >= 1, "env 2 did not fall"
    assert ref[0][0, 0] == STEPS - RESET_AT and c[0][0] == 0      # env 0: discarded, not counted, running on
    for name, a, b in zip(("running", "completed", "counts"), got, _acc(twin)):
        assert a.tobytes() == b.tobytes(), f"env.step() and the manual sequence differ in the {name} rows"
    rep = twin.gait_report(by_terrain_type=True)
    assert rep["overall"]["episodes"] == int(c[0].sum()) and rep["overall"]["falls"] == int(c[1].sum())
    assert sorted(rep["terrain_types"]) == [0] and rep["terrain_types"][0] == rep["overall"]
    assert all(v is None or np.isfinite(v) for v in rep["overall"].values())


# ---------------------------------------------------------------- off means off
def test_off_means_off():
    """A default env has no metrics tensors, the entry points refuse it with a reason, and its step()
    outputs for 10 steps are bitwise those of an env with the feature on (the metrics only read)."""
    _need_gpu()
    N, L = _lib()
    n = 65
    off = _make_env(n)
    on = _make_env(n, metrics__gait=True)
    for name in ("metrics_running", "metrics_completed", "metrics_counts", "metrics_names", "gait_report",
                 "clear_gait_metrics"):
        assert not hasattr(off, name) and hasattr(on, name), name
    assert on.metrics_names == MR.NAMES
    assert tuple(on.metrics_running.shape) == (13, n) and on.metrics_running.dtype == torch.float64
    assert tuple(on.metrics_counts.shape) == (4, n) and on.metrics_counts.dtype == torch.int32
    d = N.HgDesc()
    for tid in ("METRICS_RUN", "METRICS_DONE", "METRICS_COUNT"):
        assert L.hg_tensor(off.sim, N.T[tid], ctypes.byref(d)) == 1
    s = _stream(off)
    for call in (lambda: L.hg_metrics_sample(off.sim, s), lambda: L.hg_metrics_fold(off.sim, 0, None, s),
                 lambda: L.hg_metrics_clear(off.sim, s)):
        assert call() == 1 and b"gait metrics are off" in L.hg_last_error(off.sim)
    assert off._arena_base.numel() < on._arena_base.numel()
    for k in range(10):
        act = _actions(k, n, off.device)
        a, b = off.step(act), on.step(act)
        for x, y in zip(a[:4], b[:4]):
            assert torch.equal(x, y), f"step {k}"
    for attr in ("root_states", "dof_pos", "dof_vel", "torques", "commands", "contact_forces"):
        assert torch.equal(getattr(off, attr), getattr(on, attr)), attr
    assert int(_g(on.metrics_running)[0].sum() + _g(on.metrics_completed)[0].sum()) == 10 * n


# ---------------------------------------------------------------- runner
def _runner(env, log_dir, steps=16):
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = steps
    return OnPolicyRunner(env, class_to_dict(tcfg), log_dir=log_dir, device="cuda:0")


def test_runner_reports_gait_stats(tmp_path):
    """One learn iteration with the feature on (0.1 s episodes, so the rollout sees time-outs) puts
    finite gait_* entries into last_iteration_stats and Gait/* scalars into the log; the accumulators
    are cleared behind the read; without a log writer the figures arrive the same way; with the
    feature off the keys are absent."""
    _need_gpu()
    from humanoid.algo.ppo.on_policy_runner import _JsonlWriter
    env = _make_env(64, metrics__gait=True, env__episode_length_s=0.1)
    log_dir = str(tmp_path / "run")
    runner = _runner(env, log_dir)
    runner.writer = _JsonlWriter(log_dir)
    runner.learn(1, init_at_random_ep_len=True)
    gait = {k: v for k, v in runner.last_iteration_stats.items() if k.startswith("gait_")}
    print("runner gait stats:", gait)
    for key in ("gait_episodes", "gait_fall_rate", "gait_rms_err_vx", "gait_cost_of_transport", "gait_slip_per_metre",
                "gait_double_support_fraction", "gait_peak_torque_ratio", "gait_skipped"):
        assert key in gait, key
    assert all(np.isfinite(v) for v in gait.values()) and gait["gait_episodes"] >= 64 and gait["gait_time_outs"] >= 1
    assert gait["gait_falls"] + gait["gait_time_outs"] == gait["gait_episodes"]
    rows = [json.loads(ln) for ln in open(os.path.join(log_dir, "scalars.jsonl"))]
    tags = {r["tag"] for r in rows}
    assert {"Gait/episodes", "Gait/fall_rate", "Gait/rms_err_vx", "Gait/cost_of_transport"} <= tags
    assert not _g(env.metrics_completed).any() and not _g(env.metrics_counts).any()   # a fresh interval
    # the path without a log writer: read one iteration late, from pinned memory
    lazy = _runner(_make_env(64, metrics__gait=True, env__episode_length_s=0.1), None)
    lazy.learn(2, init_at_random_ep_len=True)
    g2 = {k: v for k, v in lazy.last_iteration_stats.items() if k.startswith("gait_")}
    assert g2["gait_episodes"] >= 64 and all(np.isfinite(v) for v in g2.values())
    # off: nothing changes
    plain = _runner(_make_env(64, env__episode_length_s=0.1), None)
    plain.learn(1, init_at_random_ep_len=True)
    assert plain.last_iteration_stats and not any(k.startswith("gait_") for k in plain.last_iteration_stats)


# ---------------------------------------------------------------- the evaluation script
def test_evaluate_script_reports_and_writes_json(tmp_path):
    """scripts/evaluate.py on a golden actor: main() runs 8 envs for 0.3 s with a fixed command and
    writes gait_report.json; evaluate() on an env with 0.2 s episodes reports completed episodes,
    every figure finite, overall equal to the one terrain type of the plane."""
    _need_gpu()
    from humanoid.scripts import evaluate as EV
    from humanoid.scripts.sim2sim import load_policy
    actor = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_trained_actor.npz")
    rep = EV.main(["--load_model", actor, "--envs", "8", "--duration", "0.3", "--command", "0.4", "0", "0",
                   "--out", str(tmp_path)])
    js = json.load(open(tmp_path / "gait_report.json"))
    assert js["settings"] == rep["settings"] and js["settings"]["steps"] == 30 and js["settings"]["command"] == [0.4, 0.0, 0.0]
    assert js["overall"] == rep["overall"] and list(js["terrain_types"]) == ["0"]
    env = _make_env(8, metrics__gait=True, env__episode_length_s=0.2)
    rep, env = EV.evaluate(load_policy(actor), duration=0.5, command=(0.4, 0.0, 0.0), env=env)
    o = rep["overall"]
    print(EV.format_report(rep))
    assert o["episodes"] >= 8 and o["falls"] + o["time_outs"] == o["episodes"] and o["skipped"] == 0
    assert all(v is not None and np.isfinite(v) for v in o.values())
    assert rep["terrain_types"][0] == o
    with pytest.raises(ValueError):
        EV.evaluate(load_policy(actor), duration=0.1, env=_make_env(2))
