"""Command curriculum and curriculum extras on the device (commands.curriculum,
extras["episode"]["max_command_x"] / ["terrain_level"]; reference humanoid_env.py:1097-1106,
1120-1129, 1146-1149) against the unchanged oracle.

The reference widens command_ranges["lin_vel_x"] inside reset_idx BEFORE that reset draws its
commands, while the same step's periodic resample (earlier in post_physics_step) still used the old
range.  The expected state of such a step is therefore assembled from two runs of
oracle/pipeline_ref.post on the same snapshot — one with the range going in, one with the range
coming out: the resetting envs' commands[:, 0:2] and the command columns 2, 3 of their newest
observation / privileged frames come from the second run, everything else from the first.  The
expected range comes from the float64 restatement of the rule pinned to the reference on the CPU
(tests/test_cmd_curriculum_rule.curriculum_rule).  Tolerances are _post_parity's own: commands
1e-5, observations 1e-4, rewards 2e-4 / 2e-5, resets and time-outs exact; the live range within
2^-23 relative of the float64 rule (one float32 rounding of the bound, one of the sum);
max_command_x equal to range[1] bit for bit."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from test_cmd_curriculum_rule import curriculum_rule
from test_gpu_parity import _make_env, _need_gpu, _oracle_cfg, _plant_episode_sums, _post_once, snapshot

pytestmark = pytest.mark.gpu

THRESH = 0.8 * 1.2 * 0.01 * 2400  # 23.04: the threshold on the mean tracking_lin_vel sum at the defaults
TLV = 20                          # tracking_lin_vel's row of the episode sums
OBS1, PRIV1 = 47, 73


def g(t):
    return t.detach().cpu().numpy().copy()


def _live_range(env):
    torch.cuda.synchronize()
    return g(env._cmd_range).astype(np.float64)


def _assert_range(env, want, label=""):
    got = _live_range(env)
    for a, b in zip(got, want):
        assert abs(a - b) <= 2.0 ** -23 * abs(b), (label, got, want)
    return got


def _cfg_with_range(env, rng):
    import pipeline_ref as PR
    from humanoid import _native as N
    c = N.HgCfg.from_buffer_copy(env._hgcfg)
    c.cmd_lin_x[0], c.cmd_lin_x[1] = float(rng[0]), float(rng[1])
    return PR.Cfg(c)


def _prepare(env, forced, mean, other, seed, steps=3):
    """A few steps, then the forced branches of _post_parity (base contact on `forced`, time-outs on
    4..7, a command resample on 8..11 and on forced[4]) and planted episode sums: tracking_lin_vel
    `mean` on average (spread around it) over the envs the oracle says reset, `other` elsewhere."""
    import pipeline_ref as PR
    for _ in range(steps):
        env.step(torch.randn(env.num_envs, 12, device="cuda:0") * 0.5)
    torch.cuda.synchronize()
    if forced:
        env.contact_forces[forced, 0, 2] = 50.0
        env.episode_length_buf[4:8] = 2400
        env.episode_length_buf[forced[4]] = 799  # a resetting env that also hits the periodic resample
    env.episode_length_buf[8:12] = 799
    _plant_episode_sums(env, seed)
    # which envs reset does not depend on the sums: ask the oracle first
    S, ho, hp = snapshot(env)
    reset = PR.post(_oracle_cfg(env), S, 1, ho, hp)[3].astype(bool)
    rid = np.nonzero(reset)[0]
    sums = np.full(env.num_envs, other, np.float32)
    sums[rid] = (mean + (np.arange(len(rid)) - (len(rid) - 1) / 2.0) * 0.125).astype(np.float32)
    env._sums[TLV].copy_(torch.from_numpy(sums).to("cuda:0"))
    torch.cuda.synchronize()
    return rid


def _mixed_oracle(env, counter, old, new):
    """pipeline_ref.post on two copies of the env's state (range `old` / range `new`), merged as
    the module docstring says.  Returns (expected dict, the two runs' states)."""
    import pipeline_ref as PR
    S, ho, hp = snapshot(env)
    runs = []
    for rng in (old, new):
        Sc, extras = copy.deepcopy(S), {}
        out = PR.post(_cfg_with_range(env, rng), Sc, counter, ho.copy(), hp.copy(), extras=extras)
        runs.append((Sc, out, extras))
    (S0, (obs0, priv0, rew0, reset0, to0, terms0), ex0), (S1, (obs1, priv1, _, reset1, _, _), _) = runs
    np.testing.assert_array_equal(reset0, reset1)
    rid = np.nonzero(reset0)[0]
    cmd, obs, priv = S0["commands"].copy(), obs0.copy(), priv0.copy()
    cmd[rid, 0:2] = S1["commands"][rid, 0:2]
    for col in (2, 3):
        obs[rid, -OBS1 + col] = obs1[rid, -OBS1 + col]
        priv[rid, -PRIV1 + col] = priv1[rid, -PRIV1 + col]
    tlv_after = S["episode_sums"]["tracking_lin_vel"] + (terms0["tracking_lin_vel"] * np.float32(
        _oracle_cfg(env).scales["tracking_lin_vel"])).astype(np.float32)
    exp = dict(S=S0, commands=cmd, obs=obs, priv=priv, rew=rew0, reset=reset0, timeout=to0, rid=rid,
               tlv_after=tlv_after, extras=ex0)
    return exp, S0, S1


def _assert_post_state(env, exp):
    np.testing.assert_array_equal(g(env.reset_buf), exp["reset"])
    np.testing.assert_array_equal(g(env.time_out_buf), exp["timeout"])
    np.testing.assert_allclose(g(env.rew_buf), exp["rew"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(g(env.commands), exp["commands"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g(env.root_states), exp["S"]["root_states"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g(env.dof_pos), exp["S"]["dof_pos"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g(env.obs_buf), exp["obs"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g(env.privileged_obs_buf), exp["priv"], rtol=1e-4, atol=1e-4)


def _rule(env, exp, counter, rng):
    c = env._hgcfg
    return curriculum_rule(exp["tlv_after"], exp["rid"], counter, rng, float(c.cmd_max_curriculum),
                           float(c.max_episode_length), float(c.reward_scale[TLV]))


def _forced(n):
    return sorted({0, 1, 2, 3, 17, n // 2, (n - 1) // 16 * 16, n - 1})


def _post_case(env, counter, mean, other, forced, seed):
    """One hg_post at `counter` on the prepared state; returns (range before, expected range,
    expected state, the two oracle runs)."""
    _prepare(env, forced, mean, other, seed)
    old = _live_range(env)
    # the decision from the oracle's sums after this step's reward (the range the merge needs is
    # the rule's own output, so run the plain oracle once for the sums, then merge)
    exp0, _, _ = _mixed_oracle(env, counter, old, old)
    new = _rule(env, exp0, counter, old)
    exp, S0, S1 = _mixed_oracle(env, counter, old, new)
    _post_once(env, counter)
    env._publish_extras()
    return old, new, exp, S0, S1


def _assert_extras(env, rng):
    ep = env.extras["episode"]
    assert "max_command_x" in ep and "terrain_level" not in ep
    assert sorted(k for k in ep if k.startswith("rew_")) == sorted("rew_" + n for n in env.reward_names)
    assert ep["max_command_x"].dim() == 0 and ep["max_command_x"].is_cuda
    assert float(ep["max_command_x"]) == float(np.float32(rng[1]))  # bit for bit the live upper bound
    assert all(np.isfinite(float(v)) for v in ep.values())


def _fires(n, forced=None):
    env = _make_env(n, commands__curriculum=True)
    assert env._hgcfg.cmd_curriculum == 1 and env._hgcfg.cmd_max_curriculum == 1.0
    np.testing.assert_array_equal(_live_range(env), np.float32([-0.3, 0.6]).astype(np.float64))
    _assert_extras(env, _live_range(env))  # the counter-0 reset of every env: zero sums, unchanged
    forced = forced or _forced(n)
    old, new, exp, S0, S1 = _post_case(env, 2400, THRESH * 1.02, 0.0, forced, 2000 + n)
    rid = exp["rid"]
    assert set(forced) <= set(rid) and not exp["reset"][8:12].any()
    assert new == pytest.approx((-0.8, 1.0), abs=1e-6)
    # the state is a discriminating one: the mean over ALL envs is below the threshold, the reset
    # commands differ between the two ranges, and so do the periodic draws of envs 8..11 (which
    # must keep the old range)
    assert exp["tlv_after"].astype(np.float64).mean() < THRESH < exp["tlv_after"][rid].astype(np.float64).mean() / 1.019
    assert np.abs(S0["commands"][rid, 0] - S1["commands"][rid, 0]).max() > 0.05
    assert np.abs(S0["commands"][8:12, 0] - S1["commands"][8:12, 0]).max() > 1e-3
    got = _assert_range(env, new, f"n={n}")
    _assert_post_state(env, exp)
    _assert_extras(env, got)
    assert env.command_ranges["lin_vel_x"] == [-0.3, 0.6]  # host copy: untouched until asked
    assert env.refresh_command_ranges() == [float(got[0]), float(got[1])] == env.command_ranges["lin_vel_x"]
    return env, forced


def test_fires_77_envs_ragged_block():
    """Case 1: 77 envs (five k_post_step blocks, the last with 13 valid lanes), counter 2400,
    resets in blocks 0, 1, 2 and on envs 64 and 76 of the ragged block, mean 2 % above."""
    _need_gpu()
    env, forced = _fires(77)
    assert {64, 76} <= set(forced) and len({e // 16 for e in forced}) >= 3


def test_below_threshold_nothing_moves():
    """Case 2: the same state with the mean 2 % below the threshold (and sums on the other envs
    that would fire it): range and commands are the plain oracle's, max_command_x the configured 0.6."""
    _need_gpu()
    env = _make_env(77, commands__curriculum=True)
    old, new, exp, S0, _ = _post_case(env, 2400, THRESH * 0.98, 40.0, _forced(77), 2077)
    assert new == tuple(old) and exp["tlv_after"].astype(np.float64).mean() > THRESH
    np.testing.assert_array_equal(exp["commands"], S0["commands"])
    np.testing.assert_array_equal(_live_range(env), old)
    _assert_post_state(env, exp)
    _assert_extras(env, old)
    assert float(env.extras["episode"]["max_command_x"]) == float(np.float32(0.6))


def test_off_step_nothing_moves():
    """Case 3: high sums at counter 2401 (no multiple of max_episode_length)."""
    _need_gpu()
    env = _make_env(77, commands__curriculum=True)
    old, new, exp, S0, _ = _post_case(env, 2401, THRESH * 1.5, 40.0, _forced(77), 2078)
    assert new == tuple(old)
    np.testing.assert_array_equal(_live_range(env), old)
    _assert_post_state(env, exp)
    _assert_extras(env, old)


def test_curriculum_step_without_resets():
    """Case 4: counter 2400 and no env resetting: no 0 / 0, the range and max_command_x carry over."""
    _need_gpu()
    env = _make_env(77, commands__curriculum=True)
    _prepare(env, [], THRESH * 1.5, 40.0, 2079, steps=1)
    old = _live_range(env)
    exp, _, _ = _mixed_oracle(env, 2400, old, old)
    assert not exp["reset"].any()
    _post_once(env, 2400)
    env._publish_extras()
    np.testing.assert_array_equal(_live_range(env), old)
    _assert_post_state(env, exp)
    _assert_extras(env, old)
    assert float(env._ep_stats[22]) == 0.0


def test_reset_idx_route_widens_before_it_draws():
    """Case 5: reset_idx([...]) (hg_reset_masked, the single-lane k_post) at counter 2400 with high
    sums: the range widens and the reset envs' commands are the widened oracle reset's."""
    _need_gpu()
    import pipeline_ref as PR
    env = _make_env(77, commands__curriculum=True)
    for _ in range(3):
        env.step(torch.randn(env.num_envs, 12, device="cuda:0") * 0.3)
    torch.cuda.synchronize()
    planted = _plant_episode_sums(env, 2080)
    ids = np.array([1, 5, 33, 64, 76])
    sums = np.full(77, 0.0, np.float32)
    sums[ids] = np.float32(THRESH * 1.02) + np.float32([-0.25, -0.125, 0.0, 0.125, 0.25])
    env._sums[TLV].copy_(torch.from_numpy(sums).to("cuda:0"))
    env.common_step_counter = 2400
    S, _, _ = snapshot(env)
    S["projected_gravity"] = g(env.projected_gravity)
    old = _live_range(env)
    c = env._hgcfg
    new = curriculum_rule(sums, ids, 2400, old, float(c.cmd_max_curriculum), float(c.max_episode_length),
                          float(c.reward_scale[TLV]))
    assert new == pytest.approx((-0.8, 1.0), abs=1e-6)
    R_old, R_new = copy.deepcopy(S), copy.deepcopy(S)
    PR.reset_envs(_cfg_with_range(env, old), R_old, ids, 2400)
    PR.reset_envs(_cfg_with_range(env, new), R_new, ids, 2400)
    assert np.abs(R_old["commands"][ids, 0] - R_new["commands"][ids, 0]).max() > 0.05
    env.reset_idx(torch.tensor(ids, device="cuda:0"))
    got = _assert_range(env, new, "reset_idx")
    keep = np.setdiff1d(np.arange(77), ids)
    np.testing.assert_allclose(g(env.commands)[ids], R_new["commands"][ids], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(g(env.commands)[keep], S["commands"][keep])
    for k in ("root_states", "dof_pos"):
        np.testing.assert_allclose(g(getattr(env, k))[ids], R_new[k][ids], rtol=1e-6, atol=1e-6, err_msg=k)
    # the command columns of the reset envs' newest frames follow (clip(cmd * obs_scales.lin_vel))
    want = np.clip(R_new["commands"][ids, 0:2] * np.float32(c.obs_lin_vel), -c.clip_observations, c.clip_observations)
    np.testing.assert_allclose(g(env.obs_buf)[ids, -OBS1 + 2:-OBS1 + 4], want, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g(env.privileged_obs_buf)[ids, -PRIV1 + 2:-PRIV1 + 4], want, rtol=1e-4, atol=1e-4)
    _assert_extras(env, got)
    assert planted.shape[0] == 22


def test_persistence_saturation_update_cfg_and_set_range():
    """Case 6: the widened range persists into a later plain step's periodic resample, survives
    hg_update_cfg, saturates at [-1, 1] after three firings, and hg_set_command_range_x /
    refresh_command_ranges round-trip."""
    _need_gpu()
    from humanoid import _native as N
    env, forced = _fires(77)
    wide = _live_range(env)
    # hg_update_cfg (the push-curriculum path) between launches: the device range is not reset
    env._hgcfg.max_push_vel_xy = 0.25
    N.check(N.lib().hg_update_cfg(env.sim, ctypes.byref(env._hgcfg), env._stream()), env.sim)
    np.testing.assert_array_equal(_live_range(env), wide)
    # a plain step (counter 2401) with a forced periodic resample: the oracle with the widened cfg
    env.episode_length_buf[8:12] = 799
    torch.cuda.synchronize()
    exp, S0, _ = _mixed_oracle(env, 2401, wide, wide)
    plain, _, _ = _mixed_oracle(env, 2401, [-0.3, 0.6], [-0.3, 0.6])
    assert np.abs(plain["commands"][8:12, 0] - exp["commands"][8:12, 0]).max() > 1e-3
    _post_once(env, 2401)
    env._publish_extras()
    _assert_post_state(env, exp)
    np.testing.assert_array_equal(_live_range(env), wide)
    _assert_extras(env, wide)
    # second and third firing: [-1, 1], then unchanged
    for k, counter in enumerate((4800, 7200)):
        old, new, exp, _, _ = _post_case(env, counter, THRESH * 1.05, 0.0, forced, 2100 + k)
        assert new == (-1.0, 1.0) and set(forced) <= set(exp["rid"])
        np.testing.assert_array_equal(_live_range(env), [-1.0, 1.0])
        _assert_post_state(env, exp)
        _assert_extras(env, [-1.0, 1.0])
    # checkpoint-resume write and the host read-back
    env.set_command_range_x(-0.55, 0.85)
    assert env.refresh_command_ranges() == [float(np.float32(-0.55)), float(np.float32(0.85))]
    assert env.command_ranges["lin_vel_x"] == [float(np.float32(-0.55)), float(np.float32(0.85))]
    assert N.lib().hg_set_command_range_x(env.sim, 0.5, -0.5, env._stream()) != 0  # lo > hi: refused


def test_fires_1001_envs_every_block_contributes():
    """Case 7: 1001 envs, a reset in each of the 63 k_post_step blocks (the last with 9 valid
    lanes): 63 blocks add to the accumulators; the rule and the patched frames on every reset env."""
    _need_gpu()
    n = 1001
    forced = sorted(set(range(5, n, 16)) | {0, 1, 2, 3, n - 1})
    assert len({e // 16 for e in forced}) == 63
    _fires(n, forced)


def test_terrain_level_extra_trimesh():
    """Case 8: mesh_type trimesh with the terrain curriculum on and forced level moves (as
    test_terrain_curriculum_parity forces them): extras["episode"]["terrain_level"] is
    mean(terrain_levels.float()) of the oracle's levels after the step, exactly; no max_command_x
    with the command curriculum off; no terrain_level key on a heightfield env."""
    _need_gpu()
    import pipeline_ref as PR
    env = _make_env(77, terrain__mesh_type="trimesh", terrain__curriculum=True)
    assert env._hgcfg.curriculum == 1 and env._hgcfg.cmd_curriculum == 0
    ep = env.extras["episode"]
    assert "terrain_level" in ep and "max_command_x" not in ep
    torch.cuda.synchronize()
    # the construction-time reset of every env folds the initial levels
    assert float(ep["terrain_level"]) == float(np.mean(g(env.terrain_levels).astype(np.float32)))
    for _ in range(3):
        env.step(torch.randn(env.num_envs, 12, device="cuda:0") * 0.3)
    torch.cuda.synchronize()
    n = 16
    env.contact_forces[0:n, 0, 2] = 50.0
    env.contact_forces[[64, 76], 0, 2] = 50.0
    env.root_states[0:4, 0] = env.env_origins[0:4, 0] + 5.0        # walked far: level up (1 -> 2)
    env.terrain_levels[0:2] = 1
    env.terrain_levels[2:4] = env.cfg.terrain.num_rows - 1         # ... past the top: re-draw
    env.root_states[4:8, :2] = env.env_origins[4:8, :2]            # stood still ...
    env.commands[4:8, 0] = 0.5                                     # ... under a command: level down (3 -> 2)
    env.terrain_levels[4:6] = 3
    env.terrain_levels[6:8] = 0                                    # ... already at 0: clip
    env.root_states[64, 0] = env.env_origins[64, 0] + 5.0          # the ragged block: up (1 -> 2)
    env.terrain_levels[64] = 1
    counter = 777
    S, ho, hp = snapshot(env)
    lv0 = S["terrain_levels"].copy()
    reset = PR.post(_oracle_cfg(env), S, counter, ho, hp)[3]
    assert reset[:n].all() and reset[64] and reset[76]
    lv = S["terrain_levels"]
    assert (lv[[0, 1, 64]] == 2).all() and (lv[4:6] == 2).all() and (lv[6:8] == 0).all()
    _post_once(env, counter)
    env._publish_extras()
    np.testing.assert_array_equal(g(env.terrain_levels), S["terrain_levels"])
    ep = env.extras["episode"]
    want = np.mean(S["terrain_levels"].astype(np.float32))
    assert want != np.mean(lv0.astype(np.float32))
    assert ep["terrain_level"].dim() == 0 and float(ep["terrain_level"]) == float(want)
    assert "max_command_x" not in ep
    # a step in which no env resets carries the value forward
    env.contact_forces[:, 0, :] = 0.0
    env.episode_length_buf[:] = 10
    torch.cuda.synchronize()
    _post_once(env, counter + 1)
    env._publish_extras()
    assert float(env._ep_stats[22]) == 0.0
    assert float(env.extras["episode"]["terrain_level"]) == float(want)
    hf = _make_env(64, terrain__mesh_type="heightfield", terrain__curriculum=True)
    assert "terrain_level" not in hf.extras["episode"] and "max_command_x" not in hf.extras["episode"]
    assert sorted(hf.extras["episode"]) == sorted("rew_" + k for k in hf.reward_names)


def test_runner_logs_max_command_x_and_resumes_the_range(tmp_path):
    """Case 9: OnPolicyRunner.learn (2 iterations, 64 envs x 8 steps, logging on) with
    commands.curriculum: the log carries Episode/max_command_x, and a checkpoint saved after a
    forced widening restores the range on resume."""
    _need_gpu()
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.algo.ppo.on_policy_runner import _JsonlWriter
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    env = _make_env(64, commands__curriculum=True)
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = 8
    log_dir = str(tmp_path / "run")
    runner = OnPolicyRunner(env, class_to_dict(tcfg), log_dir=log_dir, device="cuda:0")
    runner.writer = _JsonlWriter(log_dir)
    runner.learn(2, init_at_random_ep_len=True)
    rows = [json.loads(ln) for ln in open(os.path.join(log_dir, "scalars.jsonl"))]
    vals = [r["value"] for r in rows if r["tag"] == "Episode/max_command_x"]
    assert len(vals) == 2 and all(abs(v - 0.6) < 1e-6 for v in vals), vals  # the mean of 8 identical float32 values
    assert not any(r["tag"] == "Episode/terrain_level" for r in rows)
    # a forced widening, saved and restored into a fresh env
    env.set_command_range_x(-0.8, 1.0)
    path = os.path.join(log_dir, "forced.pt")
    runner.save(path)
    assert torch.load(path, weights_only=True)["command_range_x"] == [float(np.float32(-0.8)), 1.0]
    env2 = _make_env(64, commands__curriculum=True)
    runner2 = OnPolicyRunner(env2, class_to_dict(tcfg), log_dir=None, device="cuda:0")
    np.testing.assert_array_equal(_live_range(env2), np.float32([-0.3, 0.6]).astype(np.float64))
    runner2.load(path)
    np.testing.assert_array_equal(_live_range(env2), np.float32([-0.8, 1.0]).astype(np.float64))
    assert env2.command_ranges["lin_vel_x"] == [float(np.float32(-0.8)), 1.0]
    # and the restored range is the one the next draws use
    env2.step(torch.zeros(64, 12, device="cuda:0"))
    env2._publish_extras()
    assert float(env2.extras["episode"]["max_command_x"]) == 1.0
