"""Per-episode actuator randomisation (domain_rand.randomize_actuators, BUILD-DEFINED), CPU side:
the configuration reaches hg_cfg, and the one-env yardstick the GPU cases use is sensitive to the
randomised parameters.

The unchanged oracle judges the feature: oracle/physics_ref.c reads cfg->kp, cfg->kd and
model->armature, so a per-env copy of hg_cfg / hg_model (`env_cfg_model`) and a one-env RefSim give
the expectation of every env.  `replay_draw` restates the draw schedule of include/hgsim.h in
float32 from oracle/rng_ref (every product and sum rounded on its own, as the kernel pins them).
Both helpers are shared with tests/test_gpu_actuator_rand.py."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))

import rng_ref as R  # noqa: E402
import step_tolerance as ST  # noqa: E402

RNG_ACTUATOR = 10
f32 = np.float32


def replay_draw(hc, global_ids, counter):
    """(kp_scale, kd_scale, armature_add), each [len(global_ids), 12] float32: the rows
    k_actuator_draw writes for these global env ids at `counter` under hc's ranges."""
    ids = np.asarray(global_ids, np.uint64)
    seed = int(hc.seed)

    def quantity(first_block, rng):
        lo, hi = f32(rng[0]), f32(rng[1])
        cols = []
        for b in range(3):
            for w in R.rng4(seed, ids, counter, first_block + b, RNG_ACTUATOR):
                cols.append((lo + ((hi - lo) * R.u01(w)).astype(f32)).astype(f32))
        return np.stack(cols, axis=1)

    sp, sd = quantity(0, hc.act_kp_range), quantity(3, hc.act_kd_range)
    sm, a = quantity(6, hc.act_strength_range), quantity(9, hc.act_armature_range)
    return (sp * sm).astype(f32), (sd * sm).astype(f32), a


def env_cfg_model(hc, model, kp_scale, kd_scale, armature_add):
    """Copies of hg_cfg / hg_model with one env's (or one group's) effective actuator parameters,
    each from one float32 operation as K_step computes them."""
    from humanoid import _native as N
    c, m = N.HgCfg.from_buffer_copy(hc), N.HgModel.from_buffer_copy(model)
    for j in range(12):
        c.kp[j] = f32(hc.kp[j]) * f32(kp_scale[j])
        c.kd[j] = f32(hc.kd[j]) * f32(kd_scale[j])
        m.armature[j + 1] = f32(model.armature[j + 1]) + f32(armature_add[j])
    return c, m


def slice_state(S, idx):
    """The rows `idx` of the per-env arrays check_step reads."""
    return {k: np.asarray(S[k])[idx] for k in ("root_states", "dof_pos", "dof_vel", "lambda", "body_mass",
                                                "env_frictions")}


def test_build_hg_cfg_carries_the_actuator_fields():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    dr = cfg.domain_rand
    assert dr.randomize_actuators is False
    assert (dr.kp_range, dr.kd_range, dr.motor_strength_range, dr.added_armature_range) == (
        [0.8, 1.2], [0.8, 1.2], [0.9, 1.1], [0.0, 0.02])
    _, js = N.load_model()
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.actuator_rand == 0
    assert list(hc.act_kp_range) == [f32(0.8), f32(1.2)] and list(hc.act_kd_range) == [f32(0.8), f32(1.2)]
    assert list(hc.act_strength_range) == [f32(0.9), f32(1.1)] and list(hc.act_armature_range) == [0.0, f32(0.02)]
    dr.randomize_actuators = True
    dr.kp_range, dr.kd_range = [0.5, 0.75], [1.0, 1.5]
    dr.motor_strength_range, dr.added_armature_range = [0.25, 2.0], [0.005, 0.01]
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.actuator_rand == 1
    assert list(hc.act_kp_range) == [0.5, 0.75] and list(hc.act_kd_range) == [1.0, 1.5]
    assert list(hc.act_strength_range) == [0.25, 2.0] and list(hc.act_armature_range) == [f32(0.005), f32(0.01)]
    # the new fields and ids sit in front of the command curriculum's, which stay the last
    # (tests/test_cmd_curriculum_rule.py); every id up to ENV_ORDER keeps its value
    assert N.HgCfg.env_offset.offset < N.HgCfg.actuator_rand.offset < N.HgCfg.terrain_origins.offset
    assert [N.T[k] - N.T["ENV_ORDER"] for k in ("KP_SCALE", "KD_SCALE", "ARMATURE_ADD", "CMD_RANGE_X")] == [1, 2, 3, 4]
    import humanoid.scripts.sim2sim as S2S
    assert S2S.make_cfg("urdf", 4, duration=1.0).domain_rand.randomize_actuators is False


def test_replayed_draws_stay_in_their_ranges():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    _, js = N.load_model()
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    kp, kd, arm = replay_draw(hc, np.arange(4096), 7)
    for x in (kp, kd):
        assert x.dtype == f32 and x.min() >= f32(0.8) * f32(0.9) and x.max() <= f32(1.2) * f32(1.1) * (1 + 2.0 ** -22)
        assert 0.9 < x.mean() < 1.1 and x.std() > 0.1
    assert arm.min() >= 0.0 and arm.max() <= f32(0.02) and 0.009 < arm.mean() < 0.011
    # another counter, another env: other rows
    kp2, _, _ = replay_draw(hc, np.arange(4096), 8)
    assert (kp2 != kp).mean() > 0.99 and (kp[1:] != kp[:-1]).mean() > 0.99


@pytest.mark.parametrize("steps", [2, 24])
def test_one_env_yardstick_sees_the_actuator_parameters(steps):
    """The n = 1 yardstick of the GPU cases: on an airborne state (2 steps from the spawn) and on a
    contact state (24), with per-env rows drawn from the default ranges, check_step on a one-env
    slice with that env's hg_cfg / hg_model copy accepts an independent f32 member (no failures)
    and rejects the f32 step computed with the shared parameters — in every one of the 16 envs.
    The rows are the schedule's own draw for these envs at counter 0.  On the contact state one env
    (12) puts a joint-velocity element of the independent member outside the element tolerance, a
    discrete contact event that check_step's fp32 null builds show alike, so it passes the rule."""
    import contact_flip_rate as C
    import pipeline_ref as PR
    n = 16
    hc, model, oc, S, rng, counter = C.contact_state(n, steps=steps)
    a_ref = PR.preprocess_actions(oc, (0.5 * rng.standard_normal((n, 12))).astype(f32), S["actions"], counter)
    S["body_mass"] = S["body_mass"].reshape(-1, 1)
    S["env_frictions"] = S["env_frictions"].reshape(-1, 1)
    kp, kd, arm = replay_draw(hc, np.arange(n), 0)
    accepted = rejected = outliers = 0
    worst = 0.0
    for e in range(n):
        S1, a1 = slice_state(S, slice(e, e + 1)), a_ref[e:e + 1]
        c_e, m_e = env_cfg_model(hc, model, kp[e], kd[e], arm[e])
        member = ST.f32_members(c_e, m_e, S1, a1, ST.FIELDS, members=1, first=3)[0]
        _, rep, fails, _ = ST.check_step(c_e, m_e, S1, a1, member)
        accepted += not fails
        outliers += rep["outlier_envs"]
        if not rep["outlier_envs"]:
            worst = max(worst, max(rep["ratio"].values()))
        shared = ST.f32_members(hc, model, S1, a1, ST.FIELDS, members=1)[0]
        _, rep, fails, _ = ST.check_step(c_e, m_e, S1, a1, shared)
        rejected += bool(fails) and rep["outlier_envs"] == 1
    print(f"steps={steps}: accepted {accepted}/16 (worst multiple {worst:.2f} of K = {ST.STEP_TOL_K:g} in the envs "
          f"without an outlier element; {outliers} envs with one that the fp32 null rate covers), "
          f"shared-parameter step rejected {rejected}/16")
    assert accepted == n and rejected == n
