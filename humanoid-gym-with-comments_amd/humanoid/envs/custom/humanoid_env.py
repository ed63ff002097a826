"""XBotLFreeEnv on hg_sim: the reference env API (humanoid/envs/custom/humanoid_env.py:63-1437)
with the physics and all per-step env arithmetic running in HIP kernels.

Python keeps what the reference does once (config parsing, model load, domain-randomisation
draws at creation, reward-function bookkeeping) and the host-side step counter; every per-step
operation is one hg_step (action preprocessing + 10 physics substeps) and one hg_post
(derived state, commands, push, termination, 22 rewards, masked reset, observations, history
stacking) launched on the current stream — no host synchronisation.

Tensor attributes (root_states, dof_pos, contact_forces, rigid_state, commands, rew_buf, ...)
are zero-copy views into the simulator's SoA arena, so they read and write like the reference's
gymtorch-wrapped tensors (``root_states[:, 3:7]``, ``dof_pos[env_ids] = ...``).

``terrain.critic_heights`` (BUILD-DEFINED; the reference's concatenation, humanoid_env.py:871-874,
changes the privileged frame's width mid-run) widens every privileged frame by the measured
terrain heights under the sample grid, written on the device by the post launch's window kernel;
``num_privileged_obs`` then is ``c_frame_stack * (73 + P)`` here and on ``cfg.env``.

``depth.use_camera`` (the reference's attach_camera, humanoid_env.py:399-423; values BUILD-DEFINED)
adds a base-mounted depth camera rendered by hg_render_depth every ``depth.update_interval`` steps
into the ring ``depth_buffer``; off (the default) nothing of it exists.

``metrics.gait`` (BUILD-DEFINED) accumulates gait metrics per episode on the device: step() samples
the pre-reset state between hg_step and hg_post (hg_metrics_sample) and folds finished episodes right
after hg_post (hg_metrics_fold); ``gait_report()`` turns the accumulators into tracking errors, cost
of transport, slip, support fractions and the fall rate.  Off (the default) nothing of it exists.

``metrics.strides`` (BUILD-DEFINED, needs ``metrics.gait``) adds a per-foot stride detector to the
same two calls: lift-off, apex and touchdown of every step give swing time, foot clearance, step
length and width, touchdown force, stride length and stride time; ``stride_report()`` compares them
with ``rewards.target_feet_height`` and ``rewards.cycle_time``.  Off (the default) nothing of it
exists and the two calls launch what they did.
"""
import ctypes

import numpy as np
import torch

from humanoid import _native as N
from humanoid.envs.base.base_task import BaseTask
from humanoid.utils.helpers import class_to_dict
from humanoid.utils.math import quat_rotate_inverse, get_euler_xyz_tensor  # noqa: F401
from .humanoid_config import XBotLCfg  # noqa: F401

REWARD_NAMES = [
    "action_smoothness", "base_acc", "base_height", "collision", "default_joint_pos", "dof_acc", "dof_vel",
    "feet_air_time", "feet_clearance", "feet_contact_forces", "feet_contact_number", "feet_distance",
    "foot_slip", "joint_pos", "knee_distance", "low_speed", "orientation", "torques", "track_vel_hard",
    "tracking_ang_vel", "tracking_lin_vel", "vel_mismatch_exp",
]
assert REWARD_NAMES == sorted(REWARD_NAMES)

_TORCH_DTYPES = {0: torch.float32, 1: torch.int64, 2: torch.uint8, 3: torch.int32, 4: torch.float64}


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else None


def gait_report_row(done, counts, total_mass, gravity, dt):
    """One row of gait figures from accumulator arrays, on the host in float64.
    done: [13, n] completed-episode slot sums (HG_T_METRICS_DONE, slots _native.METRICS_NAMES);
    counts: [4, n] episodes, falls, time_outs, skipped; total_mass: [n] kg, each env's whole robot;
    gravity: m/s^2, positive; dt: the policy step.  A figure whose divisor is zero (no completed
    episode, no distance) is None."""
    # C-contiguous copies: numpy's sum order follows the memory layout, and the same envs must give
    # the same figures whether they come as the whole array or as a terrain type's selection
    d = np.ascontiguousarray(np.asarray(done, np.float64).reshape(len(N.METRICS_NAMES), -1))
    c = np.ascontiguousarray(np.asarray(counts, np.int64).reshape(len(N.METRICS_COUNT_NAMES), -1))
    m = np.asarray(total_mass, np.float64).reshape(-1)
    tot = dict(zip(N.METRICS_NAMES, d.sum(axis=1)))
    steps, dist = tot["steps"], tot["distance"]
    episodes, falls, time_outs, skipped = (int(v) for v in c.sum(axis=1))

    def rms(name):
        v = _ratio(tot[name], steps)
        return None if v is None else float(np.sqrt(v))
    weight_dist = float((m * float(gravity) * d[N.METRICS_NAMES.index("distance")]).sum())
    return {
        "episodes": episodes, "falls": falls, "time_outs": time_outs, "fall_rate": _ratio(falls, episodes),
        "skipped": skipped, "steps": int(steps),
        "rms_err_vx": rms("err_vx2"), "rms_err_vy": rms("err_vy2"), "rms_err_wz": rms("err_wz2"),
        "distance_per_episode": _ratio(dist, episodes),
        "cost_of_transport": _ratio(tot["work_pos"], weight_dist),
        "slip_per_metre": _ratio(tot["slip"], dist),
        "tilt_rms": rms("tilt2"),  # RMS of sin(angle between the base z axis and the vertical)
        "double_support_fraction": _ratio(tot["double_support"], steps),
        "flight_fraction": _ratio(tot["flight"], steps),
        "peak_torque_ratio": float(d[N.METRICS_NAMES.index("peak_torque")].max()) if episodes > 0 else None,
        "mean_torque2": _ratio(tot["torque2"], steps * dt),
        "action_rate_rms": rms("action_rate2"),
    }


def gait_report_arrays(done, counts, total_mass, gravity, dt, terrain_types=None):
    """gait_report_row over all envs; with terrain_types ([n] ints) a dict
    {"overall": row, "terrain_types": {type: row}} with one row per value present."""
    row = gait_report_row(done, counts, total_mass, gravity, dt)
    if terrain_types is None:
        return row
    d, c = np.asarray(done, np.float64), np.asarray(counts, np.int64)
    m, t = np.asarray(total_mass, np.float64).reshape(-1), np.asarray(terrain_types).reshape(-1).astype(np.int64)
    return {"overall": row,
            "terrain_types": {int(k): gait_report_row(d[:, t == k], c[:, t == k], m[t == k], gravity, dt)
                              for k in np.unique(t)}}


STRIDE_FEET = ("left", "right")  # cfg.feet_body order: the asset lists the left leg first


def _stride_row(tot, episodes, feet, target_feet_height, cycle_time):
    """The figures of one row from summed accumulator slots (a dict by _native.STRIDE_NAMES)."""
    strides, pairs = tot["strides"], tot["stride_pairs"]
    mean_swing = _ratio(tot["swing_time"], strides)
    mean_clear = _ratio(tot["clearance"], strides)
    mean_stride_time = _ratio(tot["stride_time"], pairs)

    def over(v, den):
        return None if v is None or not den > 0 else v / float(den)
    return {
        "strides": int(strides), "strides_per_episode": _ratio(strides, episodes),
        "mean_swing_time": mean_swing, "mean_clearance": mean_clear,
        "clearance_vs_target": over(mean_clear, target_feet_height),  # 1.0: the swing apex is at the target
        "mean_step_length": _ratio(tot["step_length"], strides), "mean_step_width": _ratio(tot["step_width"], strides),
        "mean_touchdown_force": _ratio(tot["touchdown_force"], strides),
        "mean_stride_length": _ratio(tot["stride_length"], pairs), "mean_stride_time": mean_stride_time,
        "stride_time_vs_cycle": over(mean_stride_time, cycle_time),  # 1.0: a stride takes rewards.cycle_time
        # touchdowns per second: each of the row's feet lands once per stride
        "cadence": None if mean_stride_time is None else over(float(feet), mean_stride_time),
        "swing_fraction": None if mean_swing is None else over(mean_swing, mean_stride_time or 0.0),
        "short_swing_fraction": _ratio(tot["short_swings"], strides + tot["short_swings"]),
    }


def stride_report_row(done, counts, dt, target_feet_height, cycle_time):
    """Stride figures from accumulator arrays, on the host in float64: {"left": row, "right": row,
    "both": row}.  done: [20, n] completed-episode stride sums (HG_T_STRIDE_DONE, foot-major, slots
    _native.STRIDE_NAMES); counts: [4, n] episodes, falls, time_outs, skipped (HG_T_METRICS_COUNT);
    dt: the policy step (the sums already carry it; kept for callers that want samples:
    mean_swing_time / dt); target_feet_height, cycle_time: rewards.target_feet_height / cycle_time.
    Means are per stride (clearance, step length and width, touchdown force, swing time) or per pair
    of consecutive touchdowns of one foot (stride length and time); swing_fraction is mean swing time
    over mean stride time; `both` adds the two asymmetries, (left - right) / their mean.  A figure
    whose divisor is zero is None."""
    ns = len(N.STRIDE_NAMES)
    d = np.ascontiguousarray(np.asarray(done, np.float64).reshape(2 * ns, -1))
    episodes = int(np.asarray(counts, np.int64).reshape(len(N.METRICS_COUNT_NAMES), -1)[0].sum())
    sums = d.sum(axis=1)
    per_foot = [dict(zip(N.STRIDE_NAMES, sums[f * ns:(f + 1) * ns])) for f in range(2)]
    rows = {name: _stride_row(per_foot[f], episodes, 1, target_feet_height, cycle_time)
            for f, name in enumerate(STRIDE_FEET)}
    both = _stride_row({k: per_foot[0][k] + per_foot[1][k] for k in N.STRIDE_NAMES}, episodes, 2, target_feet_height,
                       cycle_time)

    def asym(key):
        a, b = rows["left"][key], rows["right"][key]
        if a is None or b is None or a + b == 0:
            return None
        return (a - b) / ((a + b) / 2.0)
    both["swing_time_asymmetry"] = asym("mean_swing_time")
    both["step_length_asymmetry"] = asym("mean_step_length")
    rows["both"] = both
    return rows


def stride_report_arrays(done, counts, dt, target_feet_height, cycle_time, terrain_types=None):
    """stride_report_row over all envs; with terrain_types ([n] ints) a dict
    {"overall": rows, "terrain_types": {type: rows}} with one entry per value present."""
    rows = stride_report_row(done, counts, dt, target_feet_height, cycle_time)
    if terrain_types is None:
        return rows
    d, c = np.asarray(done, np.float64), np.asarray(counts, np.int64)
    t = np.asarray(terrain_types).reshape(-1).astype(np.int64)
    return {"overall": rows,
            "terrain_types": {int(k): stride_report_row(d[:, t == k], c[:, t == k], dt, target_feet_height, cycle_time)
                              for k in np.unique(t)}}


def critic_height_grid(cfg):
    """The base-frame sample grid of terrain.critic_heights as float32 [P, 2], x-major (the first two
    columns of _init_height_points, humanoid_env.py:314-328); None with the option off."""
    if not getattr(cfg.terrain, "critic_heights", False):
        return None
    x = np.asarray(cfg.terrain.measured_points_x, np.float32)
    y = np.asarray(cfg.terrain.measured_points_y, np.float32)
    return np.stack([np.repeat(x, len(y)), np.tile(y, len(x))], axis=1)


def build_hg_cfg(cfg, num_envs, sim_dt, seed, model_js, heightfield=None, hf_shape=(0, 0), terrain_origins=None,
                 terrain_shape=(0, 0), height_points=None):
    """XBotLCfg -> hg_cfg (include/hgsim.h).  Returns (hg_cfg, aux dict).  height_points: device
    pointer to critic_height_grid(cfg) (terrain.critic_heights; the grid itself is aux["height_grid"])."""
    c = N.HgCfg()
    c.num_envs = num_envs
    c.decimation = cfg.control.decimation
    it = getattr(cfg.sim.hg, "pgs_iterations", None)
    if it is None:
        px = cfg.sim.physx
        it = int(px.num_position_iterations) + int(getattr(px, "num_velocity_iterations", 0))
    c.pgs_iterations = max(1, int(it))
    c.fix_base_link = int(cfg.asset.fix_base_link)
    c.sim_dt = sim_dt
    c.gravity_z = cfg.sim.gravity[2]
    c.contact_offset = cfg.sim.physx.contact_offset
    c.max_depenetration_vel = cfg.sim.physx.max_depenetration_velocity
    c.baumgarte = cfg.sim.hg.baumgarte
    c.ground_friction = cfg.terrain.static_friction
    c.action_scale = cfg.control.action_scale
    c.clip_actions = cfg.normalization.clip_actions
    c.dynamic_randomization = cfg.domain_rand.dynamic_randomization
    bodies, dofs, effort, limits, velocity = N.model_names(model_js)
    kp, kd, tl, dd = [], [], [], []
    for j, name in enumerate(dofs):
        # substring match, last match wins (humanoid_env.py:285-297)
        p = d = 0.0
        for key in cfg.control.stiffness:
            if key in name:
                p, d = cfg.control.stiffness[key], cfg.control.damping[key]
        kp.append(p)
        kd.append(d)
        tl.append(effort[j] * cfg.safety.torque_limit)
        dd.append(cfg.init_state.default_joint_angles.get(name, 0.0))
    for j in range(12):
        c.kp[j], c.kd[j], c.torque_limit[j], c.default_dof_pos[j] = kp[j], kd[j], tl[j], dd[j]
    if heightfield is not None:
        c.terrain_type = 1
        c.hf_rows, c.hf_cols = hf_shape
        c.hf_horizontal_scale = cfg.terrain.horizontal_scale
        c.hf_vertical_scale = cfg.terrain.vertical_scale
        c.hf_border = cfg.terrain.border_size
        c.heightfield = heightfield
    dt = cfg.control.decimation * sim_dt
    c.frame_stack = cfg.env.frame_stack
    c.c_frame_stack = cfg.env.c_frame_stack
    c.max_episode_length = int(np.ceil(cfg.env.episode_length_s / dt))
    c.resample_interval = int(cfg.commands.resampling_time / dt)
    c.push_interval = int(np.ceil(cfg.domain_rand.push_interval_s / dt))
    c.push_robots = int(cfg.domain_rand.push_robots)
    c.add_noise = int(cfg.noise.add_noise)
    c.heading_command = int(cfg.commands.heading_command)
    c.only_positive_rewards = int(cfg.rewards.only_positive_rewards)
    c.dt = dt
    r = cfg.rewards
    c.cycle_time, c.target_joint_pos_scale, c.target_feet_height = r.cycle_time, r.target_joint_pos_scale, r.target_feet_height
    c.base_height_target, c.min_dist, c.max_dist = r.base_height_target, r.min_dist, r.max_dist
    c.tracking_sigma, c.max_contact_force = r.tracking_sigma, r.max_contact_force
    c.max_push_vel_xy, c.max_push_ang_vel = cfg.domain_rand.max_push_vel_xy, cfg.domain_rand.max_push_ang_vel
    rg = cfg.commands.ranges
    for dst, src in ((c.cmd_lin_x, rg.lin_vel_x), (c.cmd_lin_y, rg.lin_vel_y), (c.cmd_ang_yaw, rg.ang_vel_yaw),
                     (c.cmd_heading, rg.heading)):
        dst[0], dst[1] = src
    ns, os_ = cfg.noise.noise_scales, cfg.normalization.obs_scales
    c.noise_level, c.noise_dof_pos, c.noise_dof_vel = cfg.noise.noise_level, ns.dof_pos, ns.dof_vel
    c.noise_ang_vel, c.noise_quat = ns.ang_vel, ns.quat
    c.obs_lin_vel, c.obs_ang_vel, c.obs_dof_pos, c.obs_dof_vel, c.obs_quat = (os_.lin_vel, os_.ang_vel, os_.dof_pos,
                                                                              os_.dof_vel, os_.quat)
    c.clip_observations = cfg.normalization.clip_observations
    st = cfg.init_state
    for i in range(3):
        c.init_pos[i], c.init_lin_vel[i], c.init_ang_vel[i] = st.pos[i], st.lin_vel[i], st.ang_vel[i]
    for i in range(4):
        c.init_rot[i] = st.rot[i]
    scales = class_to_dict(cfg.rewards.scales)
    for k, name in enumerate(REWARD_NAMES):
        c.reward_scale[k] = scales.get(name, 0.0) * dt
    feet = [i for i, b in enumerate(bodies) if cfg.asset.foot_name in b]
    knees = [i for i, b in enumerate(bodies) if cfg.asset.knee_name in b]
    c.feet_body[0], c.feet_body[1] = feet
    c.knee_body[0], c.knee_body[1] = knees
    # 12-DOF index maps: ref-state pitch/knee/ankle-pitch, default-pose yaw/roll
    idx = {n: i for i, n in enumerate(dofs)}
    for k, n in enumerate(["left_leg_pitch_joint", "left_knee_joint", "left_ankle_pitch_joint",
                           "right_leg_pitch_joint", "right_knee_joint", "right_ankle_pitch_joint"]):
        c.ref_idx[k] = idx[n]
    for k, n in enumerate(["left_leg_roll_joint", "left_leg_yaw_joint", "right_leg_roll_joint", "right_leg_yaw_joint"]):
        c.yaw_roll_idx[k] = idx[n]
    c.seed = seed & 0xFFFFFFFFFFFFFFFF
    c.env_offset = int(getattr(cfg.env, "env_offset", 0))
    c.max_episode_length_s = cfg.env.episode_length_s
    c.terrain_env_length = cfg.terrain.terrain_length
    if terrain_origins is not None and cfg.terrain.curriculum:
        c.curriculum = 1
        c.terrain_rows, c.terrain_cols = terrain_shape
        c.terrain_origins = terrain_origins
    # command curriculum (update_command_curriculum, humanoid_env.py:1097-1106)
    c.cmd_curriculum = int(bool(getattr(cfg.commands, "curriculum", False)))
    c.cmd_max_curriculum = float(getattr(cfg.commands, "max_curriculum", 0.0))
    # gait metrics (BUILD-DEFINED, include/hgsim.h hg_cfg.gait_metrics)
    # a bit field: bit 0 the per-sample metrics, bit 1 the stride detector (metrics.strides), which needs bit 0
    c.gait_metrics = int(bool(getattr(getattr(cfg, "metrics", None), "gait", False)))
    if bool(getattr(getattr(cfg, "metrics", None), "strides", False)):
        if not c.gait_metrics:
            raise ValueError("metrics.strides needs metrics.gait: the stride detector runs inside the gait-metrics calls")
        c.gait_metrics |= 2
    # per-episode actuator randomisation (BUILD-DEFINED, include/hgsim.h hg_cfg.actuator_rand)
    dr = cfg.domain_rand
    c.actuator_rand = int(bool(getattr(dr, "randomize_actuators", False)))
    for dst, name, default in ((c.act_kp_range, "kp_range", (1.0, 1.0)), (c.act_kd_range, "kd_range", (1.0, 1.0)),
                               (c.act_strength_range, "motor_strength_range", (1.0, 1.0)),
                               (c.act_armature_range, "added_armature_range", (0.0, 0.0))):
        dst[0], dst[1] = getattr(dr, name, default)
    # measured heights in the privileged frame (BUILD-DEFINED, include/hgsim.h hg_cfg.critic_heights)
    grid = critic_height_grid(cfg)
    if grid is not None:
        c.critic_heights = len(grid)
        c.critic_height_scale = cfg.normalization.obs_scales.height_measurements
        c.critic_height_points = height_points
    aux = dict(height_grid=grid, feet=feet, knees=knees, dof_names=dofs, body_names=bodies, kp=kp, kd=kd, torque_limits=tl,
               default_dof_pos=dd, limits=limits, velocity=velocity, scales=scales)
    return c, aux



def _live(view):
    """Tag a window view handed out in place of a copy (stable_observations False): the next step
    rewrites it, so a consumer that keeps it past env.step must copy it (PPO.act does)."""
    view.hg_live_view = True
    return view

class XBotLFreeEnv(BaseTask):
    """Drop-in for the reference XBotLFreeEnv (humanoid_env.py:63)."""

    def __init__(self, cfg, sim_params, physics_engine, sim_device, headless):
        self.cfg = cfg
        self.sim_params = sim_params
        self.height_samples = None
        self.debug_viz = False
        self.init_done = False
        self.kernel_timer = None  # optional: object with start(name)/stop(name) (bench.py HIP-event timer)
        self._parse_cfg(self.cfg)
        super().__init__(cfg, sim_params, physics_engine, sim_device, headless)
        self._init_buffers()
        self._prepare_reward_function()
        # step() / get_observations() hand out tensors that stay valid across later steps, as the
        # reference's (its compute_observations allocates a new obs_buf per step,
        # humanoid_env.py:880-887): a copy of the current window stack.  OnPolicyRunner turns this
        # off — its PPO copies the stack into the rollout storage before the next step — and then
        # the returned tensors are the live strided window views, valid until the next step()
        # (a reset zeroes that env's older frames in place).
        self.stable_observations = True
        self.init_done = True
        # reset_idx(all) + compute_observations() (humanoid_env.py:176-178)
        self._launch_reset(None)
        if self._depth is not None:
            # the first frame, from the creation-time pose, in every ring slot
            self._render_depth_slot()
            for k in range(1, self._depth_len):
                self.depth_buffer[:, k].copy_(self.depth_buffer[:, 0])

    # ------------------------------------------------------------------ config
    def _parse_cfg(self, cfg):
        sim_dt = getattr(self.sim_params, "dt", None) or cfg.sim.dt
        self.sim_dt = sim_dt
        self.dt = cfg.control.decimation * sim_dt
        self.obs_scales = cfg.normalization.obs_scales
        self.reward_scales = class_to_dict(cfg.rewards.scales)
        self.command_ranges = class_to_dict(cfg.commands.ranges)
        if cfg.terrain.mesh_type not in ["heightfield", "trimesh"]:
            cfg.terrain.curriculum = False
        self.max_episode_length_s = cfg.env.episode_length_s
        self.max_episode_length = np.ceil(self.max_episode_length_s / self.dt)
        cfg.domain_rand.push_interval = np.ceil(cfg.domain_rand.push_interval_s / self.dt)

    def _prepare_reward_function(self):
        """Drop zero scales, multiply by dt; names in alphabetical order (humanoid_env.py:201-226)."""
        for key in list(self.reward_scales.keys()):
            if self.reward_scales[key] == 0:
                self.reward_scales.pop(key)
            else:
                self.reward_scales[key] *= self.dt
        self.reward_names = [n for n in self.reward_scales if n != "termination"]
        unknown = [n for n in self.reward_names if n not in REWARD_NAMES]
        if unknown:
            raise ValueError(f"reward terms without a HIP implementation: {unknown}")
        self.episode_sums = {name: self._sums[REWARD_NAMES.index(name)] for name in self.reward_names}

    # ------------------------------------------------------------------ creation
    def create_sim(self):
        """Model load, terrain, domain randomisation and the hg_sim handle
        (replaces create_sim/_create_envs, humanoid_env.py:333-524)."""
        self.up_axis_idx = 2
        self.hg = N.lib()
        hgc = self.cfg.sim.hg
        model, js = N.load_model(armature=hgc.armature, joint_friction=getattr(hgc, "joint_friction", True),
                                 self_collisions=self.cfg.asset.self_collisions == 0)
        self._model, self._model_js = model, js
        mesh = self.cfg.terrain.mesh_type
        hf_ptr, hf_shape = None, (0, 0)
        self.custom_origins = False
        if mesh == "plane":
            pass
        elif mesh in ("heightfield", "trimesh"):
            # 'trimesh' collides against the same triangulated heightfield (cells split along the
            # (i,j)-(i+1,j+1) diagonal, the tessellation of convert_heightfield_to_trimesh).
            # Every data-parallel rank must build the identical map: the generator runs on a
            # private numpy stream seeded by terrain.seed (default: the run seed), then the global
            # numpy state is restored.
            from humanoid.utils.terrain import HumanoidTerrain
            tseed = getattr(self.cfg.terrain, "seed", None)
            tseed = int(getattr(self.cfg, "seed", 5)) if tseed is None else int(tseed)
            saved = np.random.get_state()
            np.random.seed(tseed)
            try:
                self.terrain = HumanoidTerrain(self.cfg.terrain, self.num_envs)
            finally:
                np.random.set_state(saved)
            self.height_samples = torch.tensor(self.terrain.heightsamples, dtype=torch.int16, device=self.device)
            hf_ptr, hf_shape = self.height_samples.data_ptr(), tuple(self.height_samples.shape)
            self.custom_origins = True
        elif mesh is not None:
            raise ValueError("Terrain mesh type not recognised. Allowed types are [None, plane, heightfield, trimesh]")
        seed = int(getattr(self.cfg, "seed", 5))
        to_ptr, to_shape = None, (0, 0)
        if self.custom_origins:
            self.terrain_origins = torch.from_numpy(self.terrain.env_origins).to(self.device).to(torch.float).contiguous()
            to_ptr, to_shape = self.terrain_origins.data_ptr(), tuple(self.terrain_origins.shape[:2])
        # terrain.critic_heights: the sample grid lives on the device for the env's lifetime (the
        # window kernel of every post / reset launch reads it through hg_cfg.critic_height_points)
        grid = critic_height_grid(self.cfg)
        self._critic_height_xy = None if grid is None else torch.from_numpy(grid).to(self.device).contiguous()
        hp_ptr = None if grid is None else self._critic_height_xy.data_ptr()
        self._hgcfg, self._aux = build_hg_cfg(self.cfg, self.num_envs, self.sim_dt, seed, js, hf_ptr, hf_shape,
                                              to_ptr, to_shape, hp_ptr)
        nbytes = self.hg.hg_arena_bytes(ctypes.byref(self._hgcfg))
        self._arena = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._arena.data_ptr()) % 256
        self._arena_base = self._arena[off:off + nbytes]
        handle = ctypes.c_void_p()
        N.check(self.hg.hg_create(ctypes.byref(self._hgcfg), ctypes.byref(model),
                                  ctypes.c_void_p(self._arena_base.data_ptr()), ctypes.c_size_t(nbytes),
                                  ctypes.byref(handle)))
        self.sim = handle
        if mesh == "trimesh":
            # extras["episode"]["terrain_level"] (humanoid_env.py:1146-1147): the post launches fold the mean level
            N.check(self.hg.hg_publish_terrain_level(self.sim, 1), self.sim)
        self.num_dof = self.num_dofs = 12
        self.num_bodies = len(self._aux["body_names"])
        self.dof_names = self._aux["dof_names"]
        self.feet_indices = torch.tensor(self._aux["feet"], dtype=torch.long, device=self.device)
        self.knee_indices = torch.tensor(self._aux["knees"], dtype=torch.long, device=self.device)
        self.penalised_contact_indices = torch.tensor([0], dtype=torch.long, device=self.device)
        self.termination_contact_indices = torch.tensor([0], dtype=torch.long, device=self.device)
        self._wrap_all()
        if self._hgcfg.critic_heights > 0:
            # terrain.critic_heights: the privileged widths follow the window's frame slots (73 + P),
            # on the env and on its cfg instance: the runner, ActorCritic and RolloutStorage size
            # themselves from them
            self.num_privileged_obs = int(self.cfg.env.c_frame_stack) * self._priv_width
            self.cfg.env.single_num_privileged_obs = self._priv_width
            self.cfg.env.num_privileged_obs = self.num_privileged_obs
        self._get_env_origins()
        self._randomize_props()
        self._init_depth_camera()

    # ------------------------------------------------------------------ depth camera
    _depth = None  # the cfg's depth class when depth.use_camera is on

    def _init_depth_camera(self):
        """attach_camera (humanoid_env.py:399-423): a forward depth camera on the base, its pitch
        drawn per env from depth.angle.  The image is ray-marched against the terrain by
        hg_render_depth (no graphics pipeline); with depth.draw_robot, hg_render_depth_robot also
        draws the robot's legs and feet (links of the camera's own body are never drawn).  Nothing
        is created unless depth.use_camera is on."""
        d = getattr(self.cfg, "depth", None)
        self._depth_draw_robot = N.depth_draw_robot(d)  # refuses draw_robot without use_camera
        if d is None or not getattr(d, "use_camera", False):
            return
        self._depth = d
        w, h = (int(v) for v in d.original)
        self._depth_len = int(d.buffer_len)
        self._depth_interval = int(d.update_interval)
        if self._depth_len < 1 or self._depth_interval < 1:
            raise ValueError("depth.buffer_len and depth.update_interval must be >= 1")
        self._depth_cam = N.depth_cam(d, env_stride=self._depth_len * h * w)  # refuses a bad config here
        # the pitch of every global env from a creation stream of its own, sliced to this shard
        off, total = self._global_ids()
        lo, hi = (float(np.deg2rad(a)) for a in d.angle)
        u = torch.rand(total, generator=self._creation_generator(4))[off:off + self.num_envs]
        self.depth_cam_pitch = (lo + (hi - lo) * u).to(self.device, torch.float32).contiguous()
        # a physical ring: render k writes slot k % buffer_len in place
        self.depth_buffer = torch.zeros(self.num_envs, self._depth_len, h, w, dtype=torch.float32, device=self.device)
        self._depth_renders = 0
        # the public surface exists only with the camera on
        self.depth_frame = self._depth_frame
        self.render_depth = self._render_depth

    def _launch_depth(self, cam, out, env_stride, counter, draw_robot=None):
        """hg_render_depth, or hg_render_depth_robot when the robot's legs are drawn (None: depth.draw_robot)."""
        p = self.depth_cam_pitch
        if p.dtype != torch.float32 or p.shape != (self.num_envs,) or not p.is_contiguous() or p.device != self.device:
            raise ValueError(f"depth_cam_pitch must stay a contiguous float32 [{self.num_envs}] tensor on {self.device}")
        robot = self._depth_draw_robot if draw_robot is None else bool(draw_robot)
        entry = self.hg.hg_render_depth_robot if robot else self.hg.hg_render_depth
        N.check(entry(self.sim, ctypes.byref(cam), ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                      ctypes.c_int64(env_stride), ctypes.c_uint64(counter), self._stream()), self.sim)

    def _render_depth_slot(self):
        """One render into the ring's next slot (noise keyed by the step counter)."""
        slot = self._depth_renders % self._depth_len
        self._launch_depth(self._depth_cam, self.depth_buffer[:, slot], self.depth_buffer.stride(0),
                           self.common_step_counter)
        self._depth_renders += 1

    def _depth_frame(self, age=0):
        """[N, H, W] view of the frame rendered `age` renders ago (0: the latest).  An env that
        reset since keeps its pre-reset frames until the next render."""
        if not 0 <= age < self._depth_len:
            raise ValueError(f"depth_frame: age must be in [0, {self._depth_len}), got {age}")
        return self.depth_buffer[:, (self._depth_renders - 1 - age) % self._depth_len]

    def _render_depth(self, out=None, normalize=None, noise=None, draw_robot=None):
        """Render the camera now, at the current root states and joint positions, into a fresh or
        given contiguous float32 [N, H, W] tensor (the ring is not touched).  normalize / noise /
        draw_robot override depth.normalize / depth.dis_noise / depth.draw_robot; the noise is
        keyed by the step counter."""
        cam = self._depth_cam if normalize is None and noise is None else N.depth_cam(self._depth, normalize, noise)
        h, w = cam.height, cam.width
        if out is None:
            out = torch.empty(self.num_envs, h, w, dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or tuple(out.shape) != (self.num_envs, h, w) or not out.is_contiguous()
              or out.device != self.device):
            raise ValueError(f"render_depth: out must be a contiguous float32 [{self.num_envs}, {h}, {w}] tensor on "
                             f"{self.device}")
        self._launch_depth(cam, out, h * w, self.common_step_counter, draw_robot)
        return out

    # ------------------------------------------------------------------ follow-camera view
    def _view_env_ids(self, env_ids):
        """(device int32 tensor or None, n) for hg_view_shapes / hg_render_view."""
        if env_ids is None:
            return None, self.num_envs
        ids = torch.as_tensor(env_ids, device=self.device).to(torch.int32).contiguous().view(-1)
        if ids.numel() == 0 or ids.numel() > self.num_envs:
            raise ValueError(f"env_ids must name between 1 and {self.num_envs} envs, got {ids.numel()}")
        return ids, int(ids.numel())

    def default_view_cam(self, follow=True, n=1):
        """The camera of cfg.viewer: the follow camera (record_size, horizontal_fov, follow_offset,
        follow_target, far_clip; BUILD-DEFINED) or, follow=False, the world camera viewer.pos ->
        viewer.lookat."""
        v = self.cfg.viewer
        if follow:
            return N.view_cam(v.record_size, v.horizontal_fov, v.follow_offset, v.follow_target, v.far_clip, mode=1, n=n)
        return N.view_cam(v.record_size, v.horizontal_fov, v.pos, v.lookat, v.far_clip, mode=0, n=n)

    def view_shapes(self, env_ids=None):
        """World shape table [n, num_shapes, 16] of the drawn shapes (hg_view_shapes, include/hgsim.h):
        forward kinematics of the current root_states and dof_pos."""
        ids, n = self._view_env_ids(env_ids)
        out = torch.empty(n, N.VIEW_MAX_SHAPES, 16, dtype=torch.float32, device=self.device)
        ns = ctypes.c_int32(0)
        N.check(self.hg.hg_view_shapes(self.sim, None if ids is None else ctypes.c_void_p(ids.data_ptr()), n,
                                       ctypes.c_void_p(out.data_ptr()), ctypes.byref(ns), self._stream()), self.sim)
        return out[:, :ns.value]

    def render_view(self, env_ids=None, cam=None, rgb=None, depth=None, ids=None, want=("rgb",)):
        """Render robot and terrain (hg_render_view, include/hgsim.h) for env_ids (None: all envs)
        with `cam` (an _native.view_cam; None: the follow camera of cfg.viewer).  Returns the
        requested tensors in the order of `want`, a subset of ("rgb", "depth", "ids"): rgb uint8
        [n, H, W, 3], depth float32 [n, H, W] metres, ids uint8 [n, H, W]; a tensor passed as rgb /
        depth / ids is written in place and is part of the request."""
        eids, n = self._view_env_ids(env_ids)
        if cam is None:
            cam = self.default_view_cam(True, n)
        h, w = cam.height, cam.width
        N.view_cam((w, h), cam.horizontal_fov_deg, cam.eye, cam.target, cam.far_clip, cam.mode, n)  # validates
        spec = {"rgb": (rgb, torch.uint8, (n, h, w, 3)), "depth": (depth, torch.float32, (n, h, w)),
                "ids": (ids, torch.uint8, (n, h, w))}
        want = tuple(want)
        bad = [k for k in want if k not in spec]
        if bad:
            raise ValueError(f"render_view: want holds {bad}; choose from ('rgb', 'depth', 'ids')")
        bufs = {}
        for name, (given, dt, shape) in spec.items():
            if given is not None:
                if (given.dtype != dt or tuple(given.shape) != shape or not given.is_contiguous()
                        or given.device != self.device):
                    raise ValueError(f"render_view: {name} must be a contiguous {dt} {list(shape)} tensor on {self.device}")
                bufs[name] = given
            elif name in want:
                bufs[name] = torch.empty(shape, dtype=dt, device=self.device)
        if not bufs:
            raise ValueError("render_view: nothing requested")
        p = lambda k: ctypes.c_void_p(bufs[k].data_ptr()) if k in bufs else None  # noqa: E731
        N.check(self.hg.hg_render_view(self.sim, ctypes.byref(cam), None if eids is None else ctypes.c_void_p(eids.data_ptr()),
                                       n, p("rgb"), p("depth"), p("ids"), self._stream()), self.sim)
        out = tuple(bufs[k] for k in want)
        return out[0] if len(out) == 1 else out

    def _view(self, tid):
        d = N.HgDesc()
        N.check(self.hg.hg_tensor(self.sim, tid, ctypes.byref(d)), self.sim)
        dt = _TORCH_DTYPES[d.dtype]
        es = torch.empty((), dtype=dt).element_size()
        assert d.offset_bytes % es == 0
        shape = [d.shape[i] for i in range(d.ndim)]
        strides = [d.strides[i] for i in range(d.ndim)]
        return self._arena_base.view(dt).as_strided(shape, strides, d.offset_bytes // es)

    def _wrap_all(self):
        T = N.T
        self.root_states = self._view(T["ROOT_STATE"])
        self.dof_pos = self._view(T["DOF_POS"])
        self.dof_vel = self._view(T["DOF_VEL"])
        self.contact_forces = self._view(T["CONTACT_FORCES"])
        self.rigid_state = self._view(T["RIGID_STATE"])
        self.torques = self._view(T["TORQUES"])
        self.actions = self._view(T["ACTIONS"])
        self.last_actions = self._view(T["LAST_ACTIONS"])
        self.last_last_actions = self._view(T["LAST_LAST_ACTIONS"])
        self.last_dof_vel = self._view(T["LAST_DOF_VEL"])
        self.last_root_vel = self._view(T["LAST_ROOT_VEL"])
        self.commands = self._view(T["COMMANDS"])
        # observation histories: one sliding window per env row (HG_T_OBS_BUF / HG_T_PRIV_BUF); the
        # stacks are the [N, F * width] column slices at the sim's head slot (hg_obs_head), one
        # fixed strided view per head position (no tensor indexing per access)
        self._obs_win = self._view(T["OBS_BUF"])
        self._priv_win = self._view(T["PRIV_BUF"])
        hw = int(self.hg.hg_obs_window_advance(self.sim))
        fo, fp = int(self.cfg.env.frame_stack), int(self.cfg.env.c_frame_stack)
        wo, wp = self._obs_win.shape[1] // (fo - 1 + hw), self._priv_win.shape[1] // (fp - 1 + hw)
        self._obs_views = tuple(self._obs_win[:, h * wo:(h + fo) * wo] for h in range(hw))
        self._priv_views = tuple(self._priv_win[:, h * wp:(h + fp) * wp] for h in range(hw))
        self._priv_width = wp
        self.rew_buf = self._view(T["REW_BUF"])
        self._reset_u8 = self._view(T["RESET_BUF"])
        self._timeout_u8 = self._view(T["TIME_OUT_BUF"])
        self.reset_buf = self._reset_u8.view(torch.bool)
        self.time_out_buf = self._timeout_u8.view(torch.bool)
        self._ep_len = self._view(T["EPISODE_LENGTH"])
        self._sums = self._view(T["EPISODE_SUMS"])
        self.feet_air_time = self._view(T["FEET_AIR_TIME"])
        self.last_contacts = self._view(T["LAST_CONTACTS"]).view(torch.bool)
        self.feet_height = self._view(T["FEET_HEIGHT"])
        self.last_feet_z = self._view(T["LAST_FEET_Z"])
        self.env_frictions = self._view(T["ENV_FRICTION"]).unsqueeze(1)
        self.body_mass = self._view(T["BODY_MASS"]).unsqueeze(1)
        self.rand_push_force = self._view(T["PUSH_FORCE"])
        self.rand_push_torque = self._view(T["PUSH_TORQUE"])
        self.base_lin_vel = self._view(T["BASE_LIN_VEL"])
        self.base_ang_vel = self._view(T["BASE_ANG_VEL"])
        self.projected_gravity = self._view(T["PROJ_GRAVITY"])
        self.base_euler_xyz = self._view(T["BASE_EULER"])
        self.ref_dof_pos = self._view(T["REF_DOF_POS"])
        self.env_origins = self._view(T["ENV_ORIGINS"])
        self._ep_stats = self._view(T["EP_STATS"])
        self._ep_ring = self._view(T["EP_STATS_RING"])
        # the live lin_vel_x command range (commands.curriculum) and the per-launch snapshots of
        # (max_command_x, mean terrain level), rows as _ep_ring's
        self._cmd_range = self._view(T["CMD_RANGE_X"])
        self._curriculum_ring = self._view(T["CURRICULUM_RING"])
        # the per-env actuator model K_step runs with domain_rand.randomize_actuators or after
        # set_actuator_props: factors on the shared kp / kd, rotor inertia added to the model's armature
        self.kp_scale = self._view(T["KP_SCALE"])
        self.kd_scale = self._view(T["KD_SCALE"])
        self.armature_add = self._view(T["ARMATURE_ADD"])
        self.nonfinite_count = self._view(T["NONFINITE"])
        # constraint rows / contact points the solver's row budget dropped, per env, summed over
        # substeps (diagnostic; 0 in normal operation)
        self.rows_dropped = self._view(T["ROWS_DROPPED"])
        # K_step's wave-balancing state (read-only diagnostics): each env's constraint rows in the
        # latest step, and the env each half-wave runs next (a permutation within every XCD range)
        self.env_rows = self._view(T["ENV_ROWS"])
        self.env_order = self._view(T["ENV_ORDER"])
        self._gait = bool(self._hgcfg.gait_metrics)
        if self._gait:
            # metrics.gait: the accumulators ([13, N] float64 slot sums of the running episode and of
            # the completed ones, [4, N] int32 episodes / falls / time_outs / skipped) and the public
            # surface, which exists only with the option on
            self.metrics_running = self._view(T["METRICS_RUN"])
            self.metrics_completed = self._view(T["METRICS_DONE"])
            self.metrics_counts = self._view(T["METRICS_COUNT"])
            self.metrics_names = list(N.METRICS_NAMES)
            self.clear_gait_metrics = self._clear_gait_metrics
            self.gait_report = self._gait_report
            self.gait_pack = self._gait_pack
        self._strides = bool(self._hgcfg.gait_metrics & 2)
        if self._strides:
            # metrics.strides: per-foot stride sums of the running episode and of the completed ones
            # ([20, N] float64, row f * 10 + slot) and the detector's state ([16, N], row f * 8 + slot)
            self.stride_running = self._view(T["STRIDE_RUN"])
            self.stride_completed = self._view(T["STRIDE_DONE"])
            self.stride_state = self._view(T["STRIDE_STATE"])
            self.stride_names = list(N.STRIDE_NAMES)
            self.stride_report = self._stride_report

    def _global_ids(self):
        """(offset, total): this shard's envs are global ids [offset, offset + num_envs) of total."""
        off = int(getattr(self.cfg.env, "env_offset", 0))
        total = getattr(self.cfg.env, "num_envs_total", None)
        total = self.num_envs if total is None else int(total)
        if off < 0 or off + self.num_envs > total:
            raise ValueError(f"env shard [{off}, {off + self.num_envs}) outside num_envs_total={total}")
        return off, total

    def _creation_generator(self, stream):
        """Creation-time draws over ALL global envs from a private generator keyed by the run seed
        (the same on every rank), sliced to this shard; the global torch / numpy state is untouched."""
        g = torch.Generator()
        g.manual_seed((int(getattr(self.cfg, "seed", 5)) * 1000003 + stream) & 0x7FFFFFFFFFFFFFFF)
        return g

    def _get_env_origins(self):
        """Env origins (humanoid_env.py:586-611): terrain platforms, or a grid on the plane, as
        functions of the global env id."""
        off, total = self._global_ids()
        gid = torch.arange(off, off + self.num_envs)
        if self.custom_origins:
            max_init_level = self.cfg.terrain.max_init_terrain_level
            if not self.cfg.terrain.curriculum:
                max_init_level = self.cfg.terrain.num_rows - 1
            # levels/types live in the arena (int32): K_post's reset applies the curriculum
            self.terrain_levels = self._view(N.T["TERRAIN_LEVEL"])
            self.terrain_types = self._view(N.T["TERRAIN_TYPE"])
            levels = torch.randint(0, max_init_level + 1, (total,), generator=self._creation_generator(1))
            self.terrain_levels[:] = levels[off:off + self.num_envs].to(self.device, torch.int32)
            self.terrain_types[:] = torch.div(gid, (total / self.cfg.terrain.num_cols),
                                              rounding_mode="floor").to(self.device, torch.int32)
            self.max_terrain_level = self.cfg.terrain.num_rows
            self.env_origins[:] = self.terrain_origins[self.terrain_levels.long(), self.terrain_types.long()]
        else:
            num_cols = np.floor(np.sqrt(total))
            num_rows = np.ceil(total / num_cols)
            xx, yy = torch.meshgrid(torch.arange(num_rows), torch.arange(num_cols), indexing="ij")
            sp = self.cfg.env.env_spacing
            self.env_origins[:, 0] = (sp * xx.flatten()[gid]).to(self.device)
            self.env_origins[:, 1] = (sp * yy.flatten()[gid]).to(self.device)
            self.env_origins[:, 2] = 0.0

    def _randomize_props(self):
        """Creation-time DR (humanoid_env.py:528-553, 578-584): friction from 256 buckets, base mass;
        drawn for every global env and sliced to this shard."""
        dr = self.cfg.domain_rand
        off, total = self._global_ids()
        if dr.randomize_friction:
            lo, hi = dr.friction_range
            g = self._creation_generator(2)
            bucket_ids = torch.randint(0, 256, (total, 1), generator=g)[off:off + self.num_envs]
            buckets = (hi - lo) * torch.rand(256, 1, generator=g) + lo
            self.friction_coeffs = buckets[bucket_ids]
            self.env_frictions[:] = self.friction_coeffs.view(-1, 1).to(self.device)
        mass = np.full(self.num_envs, self._model.mass[0], dtype=np.float64)
        if dr.randomize_base_mass:
            lo, hi = dr.added_mass_range
            rs = np.random.RandomState((int(getattr(self.cfg, "seed", 5)) * 1000003 + 3) & 0xFFFFFFFF)
            mass += rs.uniform(lo, hi, size=total)[off:off + self.num_envs]
        self.body_mass[:] = torch.tensor(mass, dtype=torch.float32, device=self.device).view(-1, 1)

    def _init_buffers(self):
        self.common_step_counter = 0
        self.extras = {}
        self.gravity_vec = torch.tensor([0.0, 0.0, -1.0], device=self.device).repeat(self.num_envs, 1)
        self.forward_vec = torch.tensor([1.0, 0.0, 0.0], device=self.device).repeat(self.num_envs, 1)
        self.commands_scale = torch.tensor([self.obs_scales.lin_vel, self.obs_scales.lin_vel, self.obs_scales.ang_vel],
                                           device=self.device)
        self._base_p_gains = torch.tensor(self._aux["kp"], device=self.device).repeat(self.num_envs, 1)
        self._base_d_gains = torch.tensor(self._aux["kd"], device=self.device).repeat(self.num_envs, 1)
        self.torque_limits = torch.tensor(self._aux["torque_limits"], device=self.device)
        self.default_dof_pos = torch.tensor(self._aux["default_dof_pos"], device=self.device).unsqueeze(0)
        self.default_joint_pd_target = self.default_dof_pos.clone()
        lim = torch.tensor(self._aux["limits"], device=self.device)
        self.dof_pos_limits = lim * self.cfg.safety.pos_limit
        self.dof_vel_limits = torch.tensor(self._aux["velocity"], device=self.device) * self.cfg.safety.vel_limit
        self.base_init_state = torch.tensor(self.cfg.init_state.pos + self.cfg.init_state.rot + self.cfg.init_state.lin_vel
                                            + self.cfg.init_state.ang_vel, device=self.device)
        self.measured_heights = 0
        if self.cfg.terrain.measure_heights:
            self.height_points = self._init_height_points()
            self._height_xy = self.height_points[0, :, :2].contiguous()
            self.measured_heights = torch.zeros(self.num_envs, self.num_height_points, device=self.device)
        # extras["episode"] entries are views into a ring of this many post/reset snapshots
        self.episode_snapshot_rows = N.EP_RING
        self.course_gain = 1.0   # read by OnPolicyRunner.learn (on_policy_runner.py:160-162)
        self.course_ratio = 1.0

    def _init_height_points(self):
        """Base-frame sample grid (humanoid_env.py:314-328): [N, P, 3], x-major meshgrid."""
        y = torch.tensor(self.cfg.terrain.measured_points_y, device=self.device)
        x = torch.tensor(self.cfg.terrain.measured_points_x, device=self.device)
        grid_x, grid_y = torch.meshgrid(x, y, indexing="ij")
        self.num_height_points = grid_x.numel()
        points = torch.zeros(self.num_envs, self.num_height_points, 3, device=self.device)
        points[:, :, 0] = grid_x.flatten()
        points[:, :, 1] = grid_y.flatten()
        return points

    def _get_heights(self, env_ids=None):
        """Terrain heights under the sample grid (humanoid_env.py:949-985) by the HIP kernel
        hg_measure_heights: [N, P] (or [len(env_ids), P])."""
        mesh = self.cfg.terrain.mesh_type
        if mesh == "none":
            raise NameError("Can't measure height with terrain mesh type 'none'")
        if not hasattr(self, "height_points"):
            self.height_points = self._init_height_points()
            self._height_xy = self.height_points[0, :, :2].contiguous()
        out = torch.empty(self.num_envs, self.num_height_points, device=self.device)
        N.check(self.hg.hg_measure_heights(self.sim, ctypes.c_void_p(self._height_xy.data_ptr()),
                                           self.num_height_points, ctypes.c_void_p(out.data_ptr()), self._stream()),
                self.sim)
        if env_ids is not None and len(env_ids) > 0:
            return out[torch.as_tensor(env_ids, device=self.device, dtype=torch.long)]
        return out

    # ------------------------------------------------------------------ buffers with reference semantics
    @property
    def base_quat(self):
        return self.root_states[:, 3:7]

    @property
    def episode_length_buf(self):
        return self._ep_len

    @episode_length_buf.setter
    def episode_length_buf(self, value):
        # the runner re-assigns this attribute (on_policy_runner.py:104-107): copy into the sim
        self._ep_len.copy_(value.to(self._ep_len.dtype))

    @property
    def obs_buf(self):
        return self._obs_views[self.hg.hg_obs_head(self.sim)]

    @property
    def privileged_obs_buf(self):
        return self._priv_views[self.hg.hg_obs_head(self.sim)]

    @property
    def p_gains(self):
        """[N, 12] stiffness each env runs with: the configured gains x kp_scale (the configured
        gains themselves unless actuators are randomised or set_actuator_props was called)."""
        on = self._per_env_actuators or self._hgcfg.actuator_rand
        return self._base_p_gains * self.kp_scale if on else self._base_p_gains

    @property
    def d_gains(self):
        on = self._per_env_actuators or self._hgcfg.actuator_rand
        return self._base_d_gains * self.kd_scale if on else self._base_d_gains

    @property
    def dof_state(self):
        """[N*D, 2] (pos, vel) — a copy: the sim stores dof state SoA."""
        return torch.stack((self.dof_pos, self.dof_vel), dim=-1).reshape(-1, 2)

    @property
    def ref_action(self):
        return 2 * self.ref_dof_pos

    # ------------------------------------------------------------------ hot path
    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _publish_extras(self):
        # the latest post/reset launch left its EP_STATS snapshot in ring row hg_ep_stats_slot: a
        # view, intact for the next EP_RING - 1 launches (no copy kernel per step)
        # the per-term views of each ring row are built once and reused (22 fresh tensor views per
        # step cost ≈85 us of host time, a quarter of a policy step's GPU time)
        slot = self.hg.hg_ep_stats_slot(self.sim)
        cache = self.__dict__.setdefault("_ep_views", {})
        views = cache.get(slot)
        if views is None:
            stats = self._ep_ring[slot]
            views = cache[slot] = {"rew_" + n: stats[REWARD_NAMES.index(n)] for n in self.reward_names}
            # the curriculum extras under the reference's own conditions (humanoid_env.py:1146-1149)
            if self.cfg.terrain.mesh_type == "trimesh":
                views["terrain_level"] = self._curriculum_ring[slot, 1]
            if self.cfg.commands.curriculum:
                views["max_command_x"] = self._curriculum_ring[slot, 0]
        self.extras = {"episode": dict(views), "time_outs": self.time_out_buf}

    def update_push_curriculum(self, iteration):
        """Push-recovery curriculum (config 5, BUILD-DEFINED): max push velocities ramp linearly
        from the configured values to *_final over push_curriculum_iterations PPO iterations.
        Called by OnPolicyRunner.learn once per iteration; no-op unless enabled."""
        dr = self.cfg.domain_rand
        if not getattr(dr, "push_curriculum", False):
            return
        f = min(1.0, max(0.0, iteration / max(1, int(dr.push_curriculum_iterations))))
        vxy = dr.max_push_vel_xy + f * (dr.max_push_vel_xy_final - dr.max_push_vel_xy)
        vang = dr.max_push_ang_vel + f * (dr.max_push_ang_vel_final - dr.max_push_ang_vel)
        if (self._hgcfg.max_push_vel_xy, self._hgcfg.max_push_ang_vel) != (np.float32(vxy), np.float32(vang)):
            self._hgcfg.max_push_vel_xy = vxy
            self._hgcfg.max_push_ang_vel = vang
            N.check(self.hg.hg_update_cfg(self.sim, ctypes.byref(self._hgcfg), self._stream()), self.sim)
        self.push_scale = (float(self._hgcfg.max_push_vel_xy), float(self._hgcfg.max_push_ang_vel))

    def refresh_command_ranges(self):
        """Read the live lin_vel_x range (widened on the device by the command curriculum,
        humanoid_env.py:1097-1106) back into command_ranges["lin_vel_x"]: one host read, so nothing
        on the step path calls it.  Returns [lo, hi]."""
        lo, hi = self._cmd_range.tolist()
        self.command_ranges["lin_vel_x"] = [lo, hi]
        return [lo, hi]

    def set_command_range_x(self, lo, hi):
        """Set the live lin_vel_x range (checkpoint resume), ordered on the current stream."""
        N.check(self.hg.hg_set_command_range_x(self.sim, float(lo), float(hi), self._stream()), self.sim)
        self.command_ranges["lin_vel_x"] = [float(lo), float(hi)]

    _per_env_actuators = False

    def set_actuator_props(self, kp_scale=None, kd_scale=None, armature_add=None):
        """Hand-written actuator profiles: [num_envs, 12] factors on the configured kp / kd and
        rotor inertia added to the model's armature (None leaves that one alone), ordered on the
        current stream.  From this call on K_step runs its per-env variant, whether or not
        domain_rand.randomize_actuators is on (with it on, an env's rows are redrawn at its reset)."""
        ptrs, keep = [], []
        for t in (kp_scale, kd_scale, armature_add):
            if t is None:
                ptrs.append(None)
                continue
            t = torch.as_tensor(t, dtype=torch.float32, device=self.device).contiguous()
            if t.shape != (self.num_envs, 12):
                raise ValueError(f"set_actuator_props: [{self.num_envs}, 12] arrays, got {tuple(t.shape)}")
            keep.append(t)
            ptrs.append(ctypes.c_void_p(t.data_ptr()))
        N.check(self.hg.hg_set_actuator_props(self.sim, *ptrs, self._stream()), self.sim)
        self._per_env_actuators = True

    # ------------------------------------------------------------------ gait metrics
    _gait = False  # metrics.gait

    def _clear_gait_metrics(self):
        """Zero the running rows, the completed rows and the counters (ordered on the current stream)."""
        N.check(self.hg.hg_metrics_clear(self.sim, self._stream()), self.sim)

    def _gait_pack(self):
        """[19, N] float64 on the device: the completed rows, the four counters, body_mass and the
        terrain types (0 on the plane) — everything a report needs, for one device-to-host copy.
        With metrics.strides the [20, N] completed stride sums follow as rows 19..38."""
        tt = getattr(self, "terrain_types", None)
        tt = torch.zeros(1, self.num_envs, dtype=torch.float64, device=self.device) if tt is None else tt.view(1, -1)
        rows = [self.metrics_completed, self.metrics_counts.to(torch.float64),
                self.body_mass.view(1, -1).to(torch.float64), tt.to(torch.float64)]
        if self._strides:
            rows.append(self.stride_completed)
        return torch.cat(rows)

    def gait_report_from_packed(self, packed, by_terrain_type=False):
        """The report from a host copy of gait_pack() (the runner copies it asynchronously)."""
        a = np.asarray(packed, np.float64)
        done, counts, base_mass, tt = a[:13], np.rint(a[13:17]).astype(np.int64), a[17], np.rint(a[18]).astype(np.int64)
        # m_e: the model's link masses with the base's replaced by body_mass[e]; g: what K_step runs with
        links = float(sum(float(self._model.mass[b]) for b in range(1, self._model.num_bodies)))
        return gait_report_arrays(done, counts, links + base_mass, abs(float(self._hgcfg.gravity_z)),
                                  float(self._hgcfg.sim_dt) * int(self._hgcfg.decimation),
                                  tt if by_terrain_type else None)

    def _gait_report(self, by_terrain_type=False):
        """Gait figures over the episodes completed since the last clear_gait_metrics(), computed on
        the host in float64 from one device-to-host copy (a host wait: nothing on the step path
        calls it): RMS command-tracking errors, distance per episode, cost of transport
        sum(work_pos) / sum(m_e g distance_e), slip per metre, tilt, support fractions, the peak
        torque ratio, episodes, the fall rate, skipped samples; None where no episode has completed.
        by_terrain_type: {"overall": row, "terrain_types": {type: row}}."""
        return self.gait_report_from_packed(self._gait_pack().cpu().numpy(), by_terrain_type)

    # ------------------------------------------------------------------ stride statistics
    _strides = False  # metrics.strides

    def stride_report_from_packed(self, packed, by_terrain_type=False):
        """The stride report from a host copy of gait_pack() (rows 13..16 the counters, 18 the terrain
        types, 19..38 the completed stride sums)."""
        a = np.asarray(packed, np.float64)
        rw = self.cfg.rewards
        return stride_report_arrays(a[19:39], np.rint(a[13:17]).astype(np.int64),
                                    float(self._hgcfg.sim_dt) * int(self._hgcfg.decimation),
                                    float(rw.target_feet_height), float(rw.cycle_time),
                                    np.rint(a[18]).astype(np.int64) if by_terrain_type else None)

    def _stride_report(self, by_terrain_type=False):
        """Stride figures over the episodes completed since the last clear_gait_metrics(), on the host
        in float64 from one device-to-host copy (a host wait: nothing on the step path calls it):
        rows `left`, `right` and `both` of stride_report_row — strides, swing time, foot clearance
        against rewards.target_feet_height, step length and width, touchdown force, stride length,
        stride time against rewards.cycle_time, cadence, swing fraction, chatter fraction and, in
        `both`, the left / right asymmetries.  by_terrain_type: {"overall": rows, "terrain_types":
        {type: rows}}."""
        return self.stride_report_from_packed(self._gait_pack().cpu().numpy(), by_terrain_type)

    def _launch_reset(self, mask_u8):
        mp = ctypes.c_void_p(mask_u8.data_ptr()) if mask_u8 is not None else None
        N.check(self.hg.hg_reset_masked(self.sim, mp, ctypes.c_uint64(self.common_step_counter), self._stream()),
                self.sim)
        if self._gait:
            # a manual reset discards the running episode (and, with metrics.strides, the running
            # stride sums and the detector state) of the envs it resets: it is not counted
            N.check(self.hg.hg_metrics_fold(self.sim, 1, mp, self._stream()), self.sim)
        self._publish_extras()

    def step(self, actions):
        """humanoid_env.py:616-660."""
        if self.cfg.env.use_ref_actions:
            actions = actions + self.ref_action
        a = actions.detach()
        if a.dtype != torch.float32 or not a.is_contiguous() or a.device != self.device:
            a = a.to(device=self.device, dtype=torch.float32).contiguous()
        if a.shape != (self.num_envs, self.num_actions):
            raise ValueError(f"actions must be [{self.num_envs}, {self.num_actions}], got {tuple(a.shape)}")
        s = self._stream()
        kt = self.kernel_timer
        if kt is not None:
            kt.start("k_step")
        N.check(self.hg.hg_step(self.sim, ctypes.c_void_p(a.data_ptr()), ctypes.c_uint64(self.common_step_counter), s),
                self.sim)
        if kt is not None:
            kt.stop("k_step")
        if self._gait:
            # the physical, pre-reset state of this step and the commands it was driven with
            if kt is not None:
                kt.start("k_metrics_sample")
            N.check(self.hg.hg_metrics_sample(self.sim, s), self.sim)
            if kt is not None:
                kt.stop("k_metrics_sample")
        if kt is not None:
            kt.start("k_post")
        self.common_step_counter += 1
        if self.cfg.terrain.measure_heights:
            # _post_physics_step_callback (:1012-1013): after physics, before termination/reset
            N.check(self.hg.hg_measure_heights(self.sim, ctypes.c_void_p(self._height_xy.data_ptr()),
                                               self.num_height_points, ctypes.c_void_p(self.measured_heights.data_ptr()),
                                               s), self.sim)
        sink, self._rollout_sink = self._rollout_sink, None
        if sink is not None:
            # this step's post launch also writes the rollout storage slot (hg_set_rollout_sink)
            vp = ctypes.c_void_p
            N.check(self.hg.hg_set_rollout_sink(self.sim, *[vp(t.data_ptr()) if t is not None else None
                                                             for t in sink]), self.sim)
        N.check(self.hg.hg_post(self.sim, ctypes.c_uint64(self.common_step_counter), s), self.sim)
        if kt is not None:
            kt.stop("k_post")
        if self._gait:
            # the envs this post launch reset end their episode (fall or time-out)
            if kt is not None:
                kt.start("k_metrics_fold")
            N.check(self.hg.hg_metrics_fold(self.sim, 0, None, s), self.sim)
            if kt is not None:
                kt.stop("k_metrics_fold")
        self._publish_extras()
        if self._depth is not None:
            # after the post launch: the pose the observations were written from (post-reset).
            # extras["depth"] is the new frame on render steps, None between them (the convention
            # of the code attach_camera comes from)
            if self.common_step_counter % self._depth_interval == 0:
                if kt is not None:
                    kt.start("k_depth")
                self._render_depth_slot()
                if kt is not None:
                    kt.stop("k_depth")
                self.extras["depth"] = self.depth_frame(0)
            else:
                self.extras["depth"] = None
        if sink is not None:
            self.extras["rollout_sink"] = sink  # the slot tensors this step's post launch filled
        return self.get_observations(), self.get_privileged_observations(), self.rew_buf, self.reset_buf, self.extras

    _rollout_sink = None

    def set_rollout_sink(self, rewards, dones, time_outs=None):
        """The next step() also writes its rewards (float32), reset flags and time-out flags (uint8)
        into these [num_envs] device tensors — a PPO rollout-storage slot — inside its post launch
        (hg_set_rollout_sink), so the algorithm's storage write needs no launch of its own.  The
        step reports the tensors in extras["rollout_sink"]."""
        checks = [(rewards, torch.float32), (dones, torch.uint8)] + ([(time_outs, torch.uint8)] if time_outs is not None else [])
        for t, dt in checks:
            if (t is None or t.dtype != dt or t.device != self.device or t.numel() != self.num_envs
                    or not t.is_contiguous()):
                raise ValueError("set_rollout_sink: contiguous [num_envs] device tensors (float32 rewards, "
                                 "uint8 dones / time-outs)")
        self._rollout_sink = (rewards, dones, time_outs)

    def get_observations(self):
        return self.obs_buf.clone() if self.stable_observations else _live(self.obs_buf)

    def get_privileged_observations(self):
        return self.privileged_obs_buf.clone() if self.stable_observations else _live(self.privileged_obs_buf)

    def reset_idx(self, env_ids):
        """reset_idx (humanoid_env.py:1109-1163) for the given env ids, as a device mask; also
        refreshes the observation buffers of the reset envs."""
        if isinstance(env_ids, torch.Tensor) and env_ids.numel() == 0:
            return
        if len(env_ids) == 0:
            return
        mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        mask[torch.as_tensor(env_ids, device=self.device, dtype=torch.long)] = 1
        self._launch_reset(mask)

    def compute_observations(self):
        raise NotImplementedError("observations are produced by hg_post inside step()")
