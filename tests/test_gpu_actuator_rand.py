"""Per-episode actuator randomisation on the device (domain_rand.randomize_actuators, BUILD-DEFINED:
per-env kp / kd scales, motor strength and added armature; include/hgsim.h hg_cfg.actuator_rand)
against the unchanged oracle.

The draws are replayed from oracle/rng_ref by the schedule the header states
(tests/test_actuator_rand_cfg.replay_draw, float32, every product and sum rounded on its own).
K_step is judged env by env: oracle/physics_ref.c reads cfg->kp, cfg->kd and model->armature, so a
copy of hg_cfg / hg_model with one env's effective values and a one-env slice of the state give
that env's expectation under the shared rule oracle/step_tolerance.check_step — and the same check
with the shared cfg / model must fail, so a kernel that ignores the regions turns the test red."""
import ctypes

import numpy as np
import pytest
import torch

from test_actuator_rand_cfg import env_cfg_model, replay_draw, slice_state
from test_gpu_distributed import _STATE, _env as _shard_env
from test_gpu_parity import TOUCHDOWN_STEPS, _make_env, _need_gpu, _oracle_cfg, _post_once, _step_only, snapshot

pytestmark = pytest.mark.gpu

ON = dict(domain_rand__randomize_actuators=True)
FIELDS = _STATE + ("torques", "contact_forces", "rigid_state", "rows_dropped", "nonfinite_count", "time_out_buf", "_sums")
f32 = np.float32


def g(t):
    return t.detach().cpu().numpy().copy()


def _rows(env):
    """The three regions, [N, 12] each, as they stand once the stream has drained."""
    torch.cuda.synchronize()
    return g(env.kp_scale), g(env.kd_scale), g(env.armature_add)


def _assert_rows(env, ids, counter, label):
    """Rows `ids` equal the replay at `counter`: within 2^-22 max(|lo|, |hi|) of the quantity's
    range (one rounding of the product, one of the sum, fused or not), and — the kernel pins every
    rounding — bit for bit."""
    hc = env._hgcfg
    got = _rows(env)
    want = replay_draw(hc, np.asarray(ids) + int(hc.env_offset), counter)
    sm = max(abs(hc.act_strength_range[0]), abs(hc.act_strength_range[1]))
    bounds = (max(abs(hc.act_kp_range[0]), abs(hc.act_kp_range[1])) * sm,
              max(abs(hc.act_kd_range[0]), abs(hc.act_kd_range[1])) * sm,
              max(abs(hc.act_armature_range[0]), abs(hc.act_armature_range[1])))
    for name, a, b, bound in zip(("kp_scale", "kd_scale", "armature_add"), got, want, bounds):
        d = np.abs(a[ids].astype(np.float64) - b.astype(np.float64)).max() if len(ids) else 0.0
        assert d <= 2.0 ** -22 * bound, (label, name, d, bound)
        np.testing.assert_array_equal(a[ids], b, err_msg=f"{label}: {name}")
    return got


def _assert_kept(before, after, ids, label):
    keep = np.setdiff1d(np.arange(before[0].shape[0]), ids)
    for name, a, b in zip(("kp_scale", "kd_scale", "armature_add"), before, after):
        np.testing.assert_array_equal(a[keep], b[keep], err_msg=f"{label}: {name} of an env that did not reset")


def _outputs(env):
    return {"q": g(env.dof_pos), "qd": g(env.dof_vel), "root": g(env.root_states), "torques": g(env.torques),
            "rigid": g(env.rigid_state)}


def _compared_step(env, counter, scale=0.5):
    """Snapshot, one hg_step with seeded actions; returns (S, a_ref, the rows K_step ran with, gpu outputs)."""
    import pipeline_ref as PR
    S, _, _ = snapshot(env)
    rows = _rows(env)
    actions = torch.randn(env.num_envs, 12, device="cuda:0") * scale
    a_ref = PR.preprocess_actions(_oracle_cfg(env), actions.cpu().numpy(), S["actions"], counter)
    _step_only(env, actions, counter)
    np.testing.assert_allclose(g(env.actions), a_ref, rtol=1e-5, atol=1e-6)
    assert not g(env.nonfinite_count).any()
    return S, a_ref, rows, _outputs(env)


def _check_group(env, S, a_ref, gpu, idx, rows_of, label, must_reject=True):
    """check_step on the env slice `idx` with the hg_cfg / hg_model copy built from the rows
    `rows_of` (kp_scale, kd_scale, armature_add, [12] each): no failures and zero outlier envs; with
    the shared cfg / model the same candidate must fail."""
    import step_tolerance as ST
    c_e, m_e = env_cfg_model(env._hgcfg, env._model, *rows_of)
    S1, a1 = slice_state(S, idx), a_ref[idx]
    gpu1 = {k: v[idx] for k, v in gpu.items()}
    _, rep, fails, _ = ST.check_step(c_e, m_e, S1, a1, gpu1)
    print(f"{label}: multiples {({k: round(v, 2) for k, v in rep['ratio'].items()})} outlier envs {rep['outlier_envs']}"
          f"{' FAILS ' + ' | '.join(fails) if fails else ''}")
    assert not fails, f"{label}: " + " | ".join(fails)
    assert rep["outlier_envs"] == 0, (label, rep)
    if must_reject:
        _, rep0, fails0, _ = ST.check_step(env._hgcfg, env._model, S1, a1, gpu1)
        assert fails0 and rep0["outlier_envs"] >= 1, f"{label}: the shared actuator model also explains this step"
    return rep


def _per_env_parity(env, counter):
    S, a_ref, rows, gpu = _compared_step(env, counter)
    kp, kd, arm = rows
    assert (kp != 1).all() and (kd != 1).all() and (arm > 0).all()
    worst = 0.0
    for e in range(env.num_envs):
        rep = _check_group(env, S, a_ref, gpu, slice(e, e + 1), (kp[e], kd[e], arm[e]), f"env {e}")
        worst = max(worst, max(rep["ratio"].values()))
    print(f"{env.num_envs} envs checked one by one, worst multiple {worst:.2f} of K = 12")
    return S, gpu


def _force_timeouts(envs, ids):
    for env in envs:
        env.episode_length_buf[ids] = 2400
    torch.cuda.synchronize()


def test_off_is_untouched_and_neutral_rows_give_the_same_bits():
    """Case 1: 77 envs, option off, 5 steps with forced resets: the regions read 1, 1, 0 exactly.
    A second instance of the same seed with the option on and every range degenerate ([1, 1] x 3,
    [0, 0]) runs K_step's per-env variant and equals the first bit for bit (x * 1.0f, x + 0.0f)."""
    _need_gpu()
    off = _make_env(77)
    on = _make_env(77, domain_rand__kp_range=[1.0, 1.0], domain_rand__kd_range=[1.0, 1.0],
                   domain_rand__motor_strength_range=[1.0, 1.0], domain_rand__added_armature_range=[0.0, 0.0], **ON)
    assert off._hgcfg.actuator_rand == 0 and on._hgcfg.actuator_rand == 1
    gen = torch.Generator(device="cpu").manual_seed(3)
    resets = torch.zeros(77, dtype=torch.bool, device="cuda:0")
    for step in range(5):
        _force_timeouts((off, on), [step, 17 + step, 64, 76])
        a = (torch.randn(77, 12, generator=gen) * 0.5).to("cuda:0")
        outs = [e.step(a) for e in (off, on)]
        torch.cuda.synchronize()
        for name, x, y in zip(("obs", "priv", "rew", "reset"), outs[0], outs[1]):
            assert torch.equal(x, y), f"{name} differs at step {step}"
        for k in FIELDS:
            assert torch.equal(getattr(off, k), getattr(on, k)), f"{k} at step {step}"
        resets |= outs[0][3]
    assert resets[[0, 4, 17, 64, 76]].all()
    for env in (off, on):
        kp, kd, arm = _rows(env)
        assert (kp == 1).all() and (kd == 1).all() and (arm == 0).all()
    assert torch.equal(off.p_gains, on.p_gains) and torch.equal(off.d_gains, on.d_gains)


def test_draws_follow_the_schedule():
    """Case 2: 77 envs, option on.  Creation draws every env at the creation counter (0); an
    hg_post redraws exactly the envs it reset (base contact, time-out), reset_idx exactly the
    masked ones, hg_reset_masked(NULL) all of them — each at the launch's own counter; every other row keeps its bits."""
    _need_gpu()
    env = _make_env(77, **ON)
    everyone = np.arange(77)
    rows0 = _assert_rows(env, everyone, 0, "creation")
    assert len(np.unique(rows0[0])) > 900 and rows0[2].min() >= 0 and rows0[2].max() <= f32(0.02)
    assert torch.equal(env.p_gains, env._base_p_gains * env.kp_scale) and not torch.equal(env.p_gains, env._base_p_gains)
    for _ in range(3):
        env.step(torch.randn(77, 12, device="cuda:0") * 0.5)
    before = _assert_rows(env, everyone, 0, "after three steps without a reset")
    ids = np.array([0, 17, 38, 63, 64, 76])
    env.contact_forces[[0, 17, 64, 76], 0, 2] = 50.0
    env.episode_length_buf[[38, 63]] = 2400
    torch.cuda.synchronize()
    c = 1234
    _post_once(env, c)
    np.testing.assert_array_equal(np.flatnonzero(g(env.reset_buf)), ids)
    after = _assert_rows(env, ids, c, "hg_post")
    _assert_kept(before, after, ids, "hg_post")
    assert (after[0][ids] != before[0][ids]).all()
    # reset_idx: other envs, another counter; the envs the post just reset keep their rows
    ids2 = np.array([1, 5, 33, 64, 75])
    env.common_step_counter = 4321
    env.reset_idx(torch.tensor(ids2, device="cuda:0"))
    after2 = _assert_rows(env, ids2, 4321, "reset_idx")
    _assert_kept(after, after2, ids2, "reset_idx")
    assert (after2[0][ids2] != after[0][ids2]).all()
    env.common_step_counter = 777
    env._launch_reset(None)
    after3 = _assert_rows(env, everyone, 777, "hg_reset_masked(NULL)")
    assert (after3[0] != after2[0]).all()


def test_k_step_runs_each_env_with_its_rows_airborne():
    """Case 3a: 16 envs on the plane, two steps from the spawn, then the compared (airborne) step."""
    _need_gpu()
    env = _make_env(16, **ON)
    for _ in range(2):
        env.step(torch.randn(16, 12, device="cuda:0") * 0.3)
    _per_env_parity(env, 55)


def test_k_step_runs_each_env_with_its_rows_in_contact(monkeypatch):
    """Case 3b: 77 envs, TOUCHDOWN_STEPS steps, then the compared contact step, with wave balancing
    on: the env a half-wave runs comes from env_order, which is no identity here (two envs are
    lifted for the last of those steps so that the sort moves them)."""
    _need_gpu()
    monkeypatch.delenv("HG_WAVE_BALANCE", raising=False)
    env = _make_env(77, **ON)
    for _ in range(TOUCHDOWN_STEPS - 1):
        env.step(torch.randn(77, 12, device="cuda:0") * 0.3)
    # walking envs all sort into neighbouring bins, which can leave the order an identity: envs 0 and
    # 60, the first of their XCD ranges, spend the last step 0.8 m up (fewer constraint rows, a lighter
    # bin) and go to the back of their ranges, as test_wave_balancing_does_not_change_results lifts envs
    torch.cuda.synchronize()
    env.root_states[[0, 60], 2] += 0.8
    env.step(torch.randn(77, 12, device="cuda:0") * 0.3)
    torch.cuda.synchronize()
    order = g(env.env_order)
    assert sorted(order.tolist()) == list(range(77)) and (order != np.arange(77)).any()
    _, gpu = _per_env_parity(env, 91)
    from humanoid import _native as N
    lam = g(env._view(N.T["CONTACT_LAMBDA"]))[:, 0:3 * N.HG_MAX_CONTACTS:3]
    assert (lam > 0).any(axis=1).mean() >= 0.95  # a contact step


def test_k_step_runs_each_env_with_its_rows_fixed_base():
    """Case 3c: as 3a at 4 envs with asset.fix_base_link (K_step's fixed-base instantiation)."""
    _need_gpu()
    env = _make_env(4, asset__fix_base_link=True, **ON)
    assert env._hgcfg.fix_base_link == 1
    for _ in range(2):
        env.step(torch.randn(4, 12, device="cuda:0") * 0.3)
    _per_env_parity(env, 56)


def test_set_actuator_props_profiles():
    """Case 4: option off, four groups of four envs with hand-written rows (a kp scale of 0.5, a kd
    scale, both, an armature of 0.02 on the knees only): after TOUCHDOWN_STEPS each group matches
    the oracle with its group cfg / model at n = 4; the rows survive a forced reset bit for bit."""
    _need_gpu()
    env = _make_env(16)
    assert env._hgcfg.actuator_rand == 0
    kp, kd, arm = np.ones((16, 12), f32), np.ones((16, 12), f32), np.zeros((16, 12), f32)
    kp[0:4] = 0.5
    kd[4:8] = 1.5
    kp[8:12], kd[8:12], arm[8:12] = 1.25, 0.75, 0.01
    knees = [j for j, n in enumerate(env.dof_names) if "knee" in n]
    assert len(knees) == 2
    arm[12:16, knees] = 0.02
    env.set_actuator_props(kp_scale=torch.from_numpy(kp), armature_add=torch.from_numpy(arm))
    env.set_actuator_props(kd_scale=torch.from_numpy(kd).cuda())  # None leaves a region alone
    rows = _rows(env)
    for a, b in zip(rows, (kp, kd, arm)):
        np.testing.assert_array_equal(a, b)
    assert torch.equal(env.p_gains, env._base_p_gains * torch.from_numpy(kp).cuda())
    for _ in range(TOUCHDOWN_STEPS):
        env.step(torch.randn(16, 12, device="cuda:0") * 0.3)
    S, a_ref, rows, gpu = _compared_step(env, 92)
    for k in range(4):
        _check_group(env, S, a_ref, gpu, slice(4 * k, 4 * k + 4), (kp[4 * k], kd[4 * k], arm[4 * k]), f"group {k}")
    _force_timeouts((env,), [0, 5, 10, 15])
    env.step(torch.zeros(16, 12, device="cuda:0"))
    torch.cuda.synchronize()
    assert g(env.reset_buf)[[0, 5, 10, 15]].all()
    env.reset_idx(torch.tensor([1, 14], device="cuda:0"))
    for a, b in zip(_rows(env), (kp, kd, arm)):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        env.set_actuator_props(kp_scale=torch.ones(15, 12))


def test_shards_draw_by_global_env_id():
    """Case 5: shards of 13 and 77 envs at offsets 0 and 13 of a 128-env total against rows 0..89 of
    one 128-env instance, option on, short episodes: regions and state bit for bit over 40 steps."""
    _need_gpu()
    total, sizes, offs = 128, (13, 77), (0, 13)
    over = dict(env__episode_length_s=0.25, commands__resampling_time=0.1, domain_rand__push_interval_s=0.15, **ON)
    whole = _shard_env(total, 0, total, **over)
    shards = [_shard_env(n, o, total, **over) for n, o in zip(sizes, offs)]
    fields = FIELDS + ("kp_scale", "kd_scale", "armature_add")
    gen = torch.Generator(device="cpu").manual_seed(3)
    start = [whole.kp_scale[:90].clone()]
    resets = torch.zeros(90, dtype=torch.bool, device="cuda:0")
    for step in range(40):
        a = (torch.randn(total, 12, generator=gen) * 2.0).to("cuda:0")
        ow, pw, rw, dw, _ = whole.step(a)
        outs = [s.step(a[o:o + n].contiguous()) for s, n, o in zip(shards, sizes, offs)]
        torch.cuda.synchronize()
        for name, x_w, xs in (("obs", ow, [o[0] for o in outs]), ("priv", pw, [o[1] for o in outs]),
                              ("rew", rw, [o[2] for o in outs]), ("reset", dw, [o[3] for o in outs])):
            assert torch.equal(x_w[:90], torch.cat(xs)), f"{name} differs at step {step}"
        for k in fields:
            dim = 1 if k == "_sums" else 0
            parts = torch.cat([getattr(s, k) for s in shards], dim=dim)
            assert torch.equal(getattr(whole, k).narrow(dim, 0, 90), parts), f"{k} at step {step}"
        resets |= dw[:90]
    assert resets[[0, 12, 13, 89]].all()
    assert (whole.kp_scale[:90][resets] != start[0][resets]).any(dim=1).all()


def test_update_cfg_changes_ranges_and_base_gains():
    """Case 6: hg_update_cfg mid-run.  kp_range narrowed to [1.1, 1.1]: the next reset's rows are
    exactly 1.1f x the motor strength drawn; cfg.kp raised 1.5 x: the airborne per-env check passes
    with the copies built from the new base (the regions hold scales, not gains); lo > hi refused."""
    _need_gpu()
    from humanoid import _native as N
    env = _make_env(16, **ON)
    for _ in range(2):
        env.step(torch.randn(16, 12, device="cuda:0") * 0.3)
    hc = env._hgcfg
    hc.act_kp_range[0] = hc.act_kp_range[1] = 1.1
    for j in range(12):
        hc.kp[j] = f32(hc.kp[j]) * f32(1.5)
    N.check(env.hg.hg_update_cfg(env.sim, ctypes.byref(hc), env._stream()), env.sim)
    before = _rows(env)
    ids = np.array([2, 7, 15])
    env.common_step_counter = 999
    env.reset_idx(torch.tensor(ids, device="cuda:0"))
    after = _assert_rows(env, ids, 999, "narrowed kp_range")
    _assert_kept(before, after, ids, "narrowed kp_range")
    hs = N.HgCfg.from_buffer_copy(hc)  # the strength alone: kp and kd ranges degenerate at 1
    hs.act_kp_range[0] = hs.act_kp_range[1] = hs.act_kd_range[0] = hs.act_kd_range[1] = 1.0
    s_m = replay_draw(hs, ids, 999)[0]
    np.testing.assert_array_equal(after[0][ids], (f32(1.1) * s_m).astype(f32))
    env.common_step_counter = 2
    _per_env_parity(env, 57)
    bad = N.HgCfg.from_buffer_copy(hc)
    bad.act_kd_range[0], bad.act_kd_range[1] = 1.2, 0.8
    assert env.hg.hg_update_cfg(env.sim, ctypes.byref(bad), env._stream()) == 1  # HG_ERR_ARG
    assert b"lo <= hi" in env.hg.hg_last_error(env.sim)
    for field, lo in (("act_strength_range", 0.0), ("act_armature_range", -0.001)):
        bad = N.HgCfg.from_buffer_copy(hc)
        getattr(bad, field)[0] = lo
        assert env.hg.hg_update_cfg(env.sim, ctypes.byref(bad), env._stream()) == 1, field
    # the refused calls changed nothing
    _assert_kept(after, _rows(env), np.array([], int), "after refused updates")


def test_runner_trains_with_randomised_actuators():
    """Case 7: OnPolicyRunner, two iterations at 64 envs with the option on and short episodes:
    finite losses, rows redrawn by the resets of the rollout, the update graph captured."""
    _need_gpu()
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    env = _make_env(64, env__episode_length_s=0.1, **ON)
    created = _rows(env)
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = 8
    runner = OnPolicyRunner(env, class_to_dict(tcfg), log_dir=None, device="cuda:0")
    runner.learn(2, init_at_random_ep_len=True)
    st = runner.last_iteration_stats
    assert np.isfinite(st["value_loss"]) and np.isfinite(st["surrogate_loss"])
    assert torch.isfinite(env.obs_buf).all()
    now = _rows(env)
    assert (now[0] != created[0]).any(axis=1).sum() >= 1
    assert runner.alg._graphs is not None, "the second update should replay a captured graph"
