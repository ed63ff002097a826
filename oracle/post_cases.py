"""Planted rows for K_post's reward terms, termination and observation clips — TEST INFRASTRUCTURE ONLY.

Shared by tests/test_post_cases.py (CPU: coverage, bounds, mutants) and
tests/test_gpu_reward_terms.py (the kernel), in the manner of oracle/update_ref.py.

  plant(S, cfg)        a snapshot dict of a freshly made env (flat plane, default XBotLCfg, N rows)
                       -> (planted copy, Table): one env per row, every quantity a branch of
                       k_post_step reads placed at a stated margin on both sides of the branch
  reference(...)       the float32 pipeline oracle, the float64 terms (envlogic_ref.rewards with
                       dtype=float64 on a float64 derived state) and the per-term bounds
  check(got, ref, tb)  every comparison of the GPU test, as a list of violations; the CPU test runs
                       it on the float32 oracle (none allowed) and on wrong oracles (some required)

Rows are independent (one lane per env), so one hg_post runs the whole table.  N is above 64 and
no multiple of 16 (PEB = 16 envs per block: eleven blocks over the XCD remap, the last one with one valid lane).
COUNTER is no multiple of push_interval (400), so planted root velocities survive, and every
row's episode_length_buf + 1 stays off the multiples of resample_interval (800) except in the rows
that are about resampling (the time-out rows at max_episode_length = 3 x 800 are among them).

Bounds.  u = 2^-24.  Each term's bound is (number of float32 roundings) x u x (magnitude of the
summed quantities, absolute values so that cancellation is covered), plus for every fast
exponential exp(-a): exp(-a) x ((a's absolute error) + (|a| + 2) 2^-23), and the same error
propagated through every square root (d sqrt(x) <= min(dx / 2 sqrt(x), sqrt(dx)) + u sqrt(x)).  The
float64 reference is exact arithmetic on the float32 inputs and float32 constants in this sense.
"""
import copy

import numpy as np

import envlogic_ref as E
import pipeline_ref as PR

f32, f64 = np.float32, np.float64
U = 2.0 ** -24

N = 161          # 10 full blocks of 16 + one with a single env
COUNTER = 1201   # no multiple of push_interval
MARGIN = 1e-3    # default relative margin to a threshold
DISCRETE = ("collision", "feet_air_time", "feet_clearance", "feet_contact_number", "low_speed")
CMD_TERMS = ("low_speed", "track_vel_hard", "tracking_ang_vel", "tracking_lin_vel")
NAMES = E.REWARD_NAMES


# ------------------------------------------------------------------------------------------ float64 math
def _rot_inv64(q, v):
    q, v = q.astype(f64), v.astype(f64)
    qw, qv = q[:, 3:4], q[:, :3]
    return v * (2.0 * qw ** 2 - 1.0) - np.cross(qv, v) * qw * 2.0 + qv * np.sum(qv * v, 1, keepdims=True) * 2.0


def _apply64(q, v):
    q, v = q.astype(f64), v.astype(f64)
    t = np.cross(q[:, :3], v) * 2.0
    return v + q[:, 3:] * t + np.cross(q[:, :3], t)


def _wrap64(a):
    a = a - 2 * np.pi * np.floor(a / (2 * np.pi))
    return np.where(a > np.pi, a - 2 * np.pi, a)


def _euler64(q):
    x, y, z, w = [q[:, i].astype(f64) for i in range(4)]
    roll = np.arctan2(2.0 * (w * x + y * z), w * w - x * x - y * y + z * z)
    pitch = np.arcsin(np.clip(2.0 * (w * y - z * x), -1, 1))
    yaw = np.arctan2(2.0 * (w * z + x * y), w * w + x * x - y * y - z * z)
    return np.stack([_wrap64(roll), _wrap64(pitch), _wrap64(yaw)], 1)


def quat_rpy(roll, pitch, yaw):
    """(x, y, z, w) of the intrinsic z-y-x rotation, float64."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


# ------------------------------------------------------------------------------------------ the table
class Table:
    """groups: name -> row indices; clip: (row, "o" | "p", column, sign) frame entries that must be
    exactly sign x clip_observations; inside: (row, table, column) partners just inside the clip;
    resample: rows whose commands are redrawn (excluded from the command-dependent terms and the
    total: their commands are a Philox replay, not a planted value)."""

    def __init__(self):
        self.groups, self.clip, self.inside, self.rows = {}, [], [], []

    def idx(self, *names):
        return np.array(sorted(set(i for n in names for i in self.groups.get(n, []))), dtype=np.int64)


def _unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


def _row_specs(cfg):
    """The planted rows as (group, fields).  Fields are applied by plant() in a fixed order."""
    P = cfg.P
    mx = int(P.max_episode_length)
    LEFT, RIGHT, DOUBLE = 10, 40, 32      # episode_length_buf + 1: sin = 0.83, -0.71, ~0
    R = []
    add = lambda g, **kw: R.append((g, kw))  # noqa: E731
    d1, d2 = _unit([0.6, -0.5, 0.62]), _unit([-0.3, 0.7, 0.4])
    # --- termination and collision: base contact-force norm on both sides of 0.1 and 1.0
    for nrm in (0.09, 0.11, 0.99, 1.01):
        for k, d in enumerate((d1, d2)):
            add("base_force", base_cf=nrm * d, ep1=LEFT + 7 * k, sums=nrm > 1)
    for ep in (mx - 2, mx - 1, mx):       # stored value; + 1 in the launch; only mx + 1 > mx resets
        add("timeout", ep1=ep + 1, sums=ep == mx)
        add("timeout", ep1=ep + 1, sums=ep == mx, base_cf=0.05 * d2, foot_cf=[(3, 2, 300), (0, 0, 0)])
    add("timeout", ep1=mx + 1, base_cf=1.01 * d1, sums=True)
    add("timeout", ep1=mx + 1, base_cf=0.11 * d2, sums=True)
    # --- gait: a whole 64-step cycle in steps of at most 4, with the window edges
    for k, ep1 in enumerate((1, 2, 5, 9, 13, 17, 21, 25, 29, 31, 32, 33, 37, 41, 45, 49, 53, 57, 61, 63)):
        add("gait", ep1=ep1, foot_cf=[(3, -2, 300), (0, 0, 0)] if k % 2 else [(0, 0, 0), (-4, 1, 250)])
    for ep1 in (LEFT, RIGHT, DOUBLE):
        add("gait_reset", ep1=ep1, base_cf=1.01 * d2, sums=True)
    # --- feet contact: fz on both sides of 5 on each foot, lateral components that put the norm above 5
    for ep1 in (LEFT, RIGHT):
        for fz0, fz1 in ((4.99, 300), (5.01, 300), (300, 4.99), (300, 5.01)):
            add("contact", ep1=ep1, foot_cf=[(2, 1, fz0), (-1.5, 2, fz1)])
    # --- feet_contact_forces (norm against 700 and 700 + 400) on the base_height rows (root z so
    #     that the argument is +-5e-4 / +-0.05, stance left / right / double, unequal foot heights)
    fdir = _unit([0.3, -0.2, 0.93])
    forces = [(600, 300), (900, 300), (1000, 800), (1300, 300), (300, 1300), (1300, 1500), (699, 701), (1102, 1098),
              (701, 699), (1098, 1102), (1500, 1300), (650, 1090)]
    k = 0
    for ep1 in (LEFT, RIGHT, DOUBLE):
        for arg in (5e-4, -5e-4, 0.05, -0.05):
            n0, n1 = forces[k]
            add("height_force", ep1=ep1, foot_z=(0.08, 0.13), bh_arg=arg, foot_cf=[n0 * fdir, n1 * fdir * np.array([-1, 1, 1])])
            k += 1
    # --- feet_air_time: {0, 0.2, 0.495, 0.6} x {contact, last_contacts only, none} on the swing
    #     foot; the stance foot carries "stance only" with another air time
    other = (0.3, 0.0, 0.6, 0.495)
    for f, ep1 in ((0, RIGHT), (1, LEFT)):
        for kv, val in enumerate((0.0, 0.2, 0.495, 0.6)):
            for cond in ("contact", "last", "none"):
                fat, lc, cfz = [0.0, 0.0], [False, False], [(0, 0, 0), (0, 0, 0)]
                fat[f], fat[1 - f] = val, other[kv]
                lc[f] = cond == "last"
                if cond == "contact":
                    cfz[f] = (1, -1, 300)
                add("air_time", ep1=ep1, fat=fat, lc=lc, foot_cf=cfz)
    # --- feet_clearance: |feet_height + (fz - last_feet_z) - target| at 0.009 / 0.011, above and
    #     below, stance foot and swing foot, with and without contact
    for ep1 in (LEFT, RIGHT):
        for con in (False, True):
            for da, db in ((0.009, -0.011), (-0.009, 0.011), (0.011, 0.009), (-0.011, -0.009)):
                tgt = float(f32(P.target_feet_height))
                add("clearance", ep1=ep1, fht=(0.03, 0.03), lfz=(0.02, 0.02), foot_z=(0.05 + 0.02 + tgt - 0.03 + da, 0.05 + 0.02 + tgt - 0.03 + db),
                    foot_cf=[(1, 1, 300), (-1, 2, 200)] if con else [(0, 0, 0), (0, 0, 0)])
    # --- feet / knee distance, default_joint_pos (yaw / roll sum against 0.1) and joint_pos
    #     (|q - ref| against 0.5) on the same rows: the terms read disjoint inputs
    lo, hi, kh = float(f32(P.min_dist)), float(f32(P.max_dist)), float(f32(P.max_dist)) / 2
    dist = [(0.15, 0.15), (0.35, 0.22), (0.6, 0.3), (1.2, 0.9), (lo * 0.998, lo * 1.002), (lo * 1.002, lo * 0.998),
            (hi * 0.998, kh * 1.002), (hi * 1.002, kh * 0.998), ((hi + 0.5) * 0.998, (kh + 0.5) * 1.002), ((hi + 0.5) * 1.002, (kh + 0.5) * 0.998)]
    yaw_roll = [(0.09, "both"), (0.11, "both"), (0.09, "left"), (0.11, "left"), (0.09, "right"), (0.11, "right"),
                (0.0998, "left"), (0.1002, "right"), (0.3, "left"), (0.05, "right")]
    jp = [0.49, 0.51, 0.3, 0.8, 0.499, 0.501, 0.1, 1.5, 0.45, 0.55]
    for k in range(10):
        add("dist_joint", ep1=LEFT + 3 * k, feet_d=dist[k][0], knee_d=dist[k][1], yaw_roll=yaw_roll[k], jp_norm=jp[k])
    # --- low_speed: base-frame v_x at 0.49 / 0.51 / 1.19 / 1.21 |cmd_x|, |cmd_x| on both sides of
    #     the 0.1 gate, both signs, some rows through a yawed or pitched root quaternion
    k = 0
    for cx in (0.09, 0.11):
        for sgn in (1.0, -1.0):
            for ratio in (0.49, 0.51, 1.19, 1.21):
                rpy = (0, 0, 0.7) if k % 4 == 1 else ((0, 0.3, 0) if k % 4 == 3 else (0, 0, 0))
                add("low_speed", ep1=LEFT + k, cmd={0: sgn * cx}, vb=(sgn * ratio * cx, 0.05, -0.02), rpy=rpy)
                k += 1
    for cx, vx, rpy in ((0.3, -0.3, (0, 0, 0)), (-0.2, 0.15, (0, 0, -0.4)), (0.3, 0.0, (0, 0, 0)), (0.0, 0.2, (0, 0, 0)),
                        (0.0, 0.0, (0, 0, 0)), (-0.3, -0.2, (0.1, -0.2, 0.5))):
        add("low_speed", ep1=RIGHT + k, cmd={0: cx}, vb=(vx, -0.04, 0.03), rpy=rpy)
        k += 1
    # --- tracking terms, orientation, vel_mismatch_exp, base_acc with exponents of order 1; the
    #     heading command through a yawed root, saturated at +1 / -1 and on both sides of 1
    for k, (c3, rpy) in enumerate(((2.5, (0, 0, 0)), (-2.5, (0.05, -0.04, 0.3)), (1.0, (-0.06, 0.03, -0.5)), (-3.0, (0.02, 0.05, 3.0)),
                                   (1.98, (0, 0, 0)), (2.02, (0, 0, 0)), (-1.98 + 0.4, (0.03, 0.0, 0.4)), (-2.02 + 0.4, (0.0, -0.05, 0.4)))):
        add("tracking", ep1=RIGHT + 2 * k, cmd={0: 0.4, 1: -0.1, 3: c3}, rpy=rpy, vb=(0.4 + 0.15, -0.1 - 0.1, 0.3),
            wb=(0.1, -0.15, 0.2 + 0.1 * k), lrv_delta=(0.1, -0.1, 0.15, 0.1, -0.12, 0.08))
    # --- total reward: clearly negative (collision + foot forces, with and without reset) and the
    #     only_positive_rewards clip
    for k in range(4):
        add("negative_reset", ep1=LEFT + k, base_cf=(1.01 + 0.5 * k) * d1, sums=True, foot_cf=[1300 * fdir, 1500 * fdir],
            cmd={0: 0.3}, vb=(-0.3, 0.0, 0.2))
    for k in range(2):
        add("negative", ep1=RIGHT + k, base_cf=0.99 * d2, foot_cf=[(1200 + 100 * k) * fdir, 1500 * fdir], cmd={0: 0.3}, vb=(-0.3, 0.0, 0.2))
    # --- observation clips: every entry beyond the clip has a partner just inside
    add("clip", qd={0: 380.0, 5: -380.0, 7: 350.0, 11: -350.0})
    add("clip", act={1: 18.0, 2: 25.0, 3: -25.0, 4: 17.5, 9: -18.0, 10: -17.5})
    add("clip", wb=(25.0, -25.0, 17.5))
    add("clip", wb=(-17.5, 19.0, -19.0))
    add("clip", q={2: 20.0, 3: -20.0, 8: 17.5, 9: -17.5})
    add("clip", pf=(20.0, -20.0), pt=(25.0, -19.0, 17.9))
    add("clip", pf=(17.5, -17.5), pt=(-25.0, 19.0, -17.9))
    add("clip", mass=600.0, fric=20.0)
    add("clip", mass=530.0, fric=17.5)
    add("clip", mass=-600.0, fric=-20.0)
    add("clip", vb=(10.0, -10.0, 8.9))
    # --- resample: episode_length_buf + 1 on a multiple of resample_interval, with and without reset
    ri = int(cfg.c.resample_interval)
    add("resample", ep1=ri)
    add("resample", ep1=2 * ri)
    add("resample", ep1=ri, base_cf=1.01 * d2, sums=True)
    return R


def plant(S, cfg):
    """(planted copy of S, Table).  Keeps env_frictions, body_mass, env_origins and the solver state
    of S; every field a reward term, the termination or a frame reads is overwritten for all N rows
    with a neutral base line (off every threshold) and then with the rows of _row_specs."""
    n = S["root_states"].shape[0]
    assert n == N, (n, N)
    L = cfg.L
    A = copy.deepcopy(S)
    r = np.random.RandomState(20260)
    fe, kn = list(L.feet), list(L.knees)
    default = np.broadcast_to(cfg.default[None, :], (n, 12))
    A["root_states"] = np.zeros((n, 13), f32)
    A["root_states"][:, :2] = S["env_origins"][:, :2]
    A["root_states"][:, 2] = 0.95
    A["root_states"][:, 6] = 1.0
    A["dof_pos"] = (default + r.uniform(-0.05, 0.05, (n, 12))).astype(f32)
    A["dof_pos"][:, list(L.yaw_roll)] = (default[:, list(L.yaw_roll)] + r.uniform(-0.02, 0.02, (n, 4))).astype(f32)
    A["ref_dof_pos"] = r.uniform(-0.03, 0.03, (n, 12)).astype(f32)
    A["dof_vel"] = r.uniform(-0.5, 0.5, (n, 12)).astype(f32)
    A["last_dof_vel"] = (A["dof_vel"] + r.uniform(-0.05, 0.05, (n, 12))).astype(f32)
    A["actions"] = r.uniform(-0.3, 0.3, (n, 12)).astype(f32)
    A["last_actions"] = r.uniform(-0.3, 0.3, (n, 12)).astype(f32)
    A["last_last_actions"] = r.uniform(-0.3, 0.3, (n, 12)).astype(f32)
    A["torques"] = r.uniform(-10, 10, (n, 12)).astype(f32)
    A["contact_forces"] = np.zeros((n, 13, 3), f32)
    A["contact_forces"][:, fe[0]] = (3, -2, 300)
    A["contact_forces"][:, fe[1]] = (-4, 1, 250)
    A["rigid_state"] = r.uniform(-0.2, 0.2, (n, 13, 13)).astype(f32)
    A["rigid_state"][:, fe[0], :3] = (0.02, 0.15, 0.06)
    A["rigid_state"][:, fe[1], :3] = (-0.03, -0.17, 0.07)
    A["rigid_state"][:, fe[0], 10:12] = (0.3, -0.2)
    A["rigid_state"][:, fe[1], 10:12] = (-0.1, 0.5)
    A["rigid_state"][:, kn[0], :2] = (0.05, 0.11)
    A["rigid_state"][:, kn[1], :2] = (0.04, -0.10)
    A["commands"] = np.tile(np.array([0.3, 0.1, 0.0, 0.2], f32), (n, 1))
    A["episode_length_buf"] = (3 + (np.arange(n) * 7) % 55).astype(S["episode_length_buf"].dtype)
    A["feet_air_time"] = np.zeros((n, 2), f32)
    A["last_contacts"] = np.zeros((n, 2), bool)
    A["feet_height"] = np.tile(np.array([0.03, 0.04], f32), (n, 1))
    A["last_feet_z"] = np.tile(np.array([0.008, 0.018], f32), (n, 1))
    A["rand_push_force"] = np.array(S["rand_push_force"], f32)
    A["rand_push_force"][:, :2] = (0.1, -0.2)
    A["rand_push_torque"] = np.tile(np.array([0.05, -0.03, 0.02], f32), (n, 1))
    A["episode_sums"] = {nm: np.zeros(n, f32) for nm in NAMES}
    vb = np.tile(np.array([0.27, 0.05, -0.02]), (n, 1))
    wb = np.tile(np.array([0.03, -0.02, 0.05]), (n, 1))
    lrv_delta = np.tile(np.array([0.05, -0.04, 0.03, 0.02, -0.05, 0.04]), (n, 1))
    rpy = np.zeros((n, 3))
    bh_arg = np.full(n, -0.005)

    tb = Table()
    specs = _row_specs(cfg)
    assert len(specs) <= n, len(specs)
    specs += [("neutral", {})] * (n - len(specs))
    sums_rng = np.random.RandomState(977)
    for i, (g, kw) in enumerate(specs):
        tb.groups.setdefault(g, []).append(i)
        tb.rows.append(kw)
        kw = dict(kw)
        if "ep1" in kw:
            A["episode_length_buf"][i] = kw.pop("ep1") - 1
        if "base_cf" in kw:
            A["contact_forces"][i, L.base] = kw.pop("base_cf")
        if "foot_cf" in kw:
            for f, v in enumerate(kw.pop("foot_cf")):
                A["contact_forces"][i, fe[f]] = v
        if "foot_z" in kw:
            A["rigid_state"][i, fe, 2] = kw.pop("foot_z")
        for key, field in (("fat", "feet_air_time"), ("lc", "last_contacts"), ("fht", "feet_height"), ("lfz", "last_feet_z"),
                           ("pt", "rand_push_torque")):
            if key in kw:
                A[field][i] = kw.pop(key)
        if "pf" in kw:
            A["rand_push_force"][i, :2] = kw.pop("pf")
        if "mass" in kw:
            A["body_mass"][i] = kw.pop("mass")
        if "fric" in kw:
            A["env_frictions"][i] = kw.pop("fric")
        for key, field in (("q", "dof_pos"), ("qd", "dof_vel"), ("act", "actions"), ("cmd", "commands")):
            for j, v in kw.pop(key, {}).items():
                A[field][i, j] = v
        if "feet_d" in kw:   # planar distance d along u, offsets in x and y on both bodies
            u, c = np.array([0.6, 0.8]), np.array([0.13, -0.07])
            d = kw.pop("feet_d")
            A["rigid_state"][i, fe[0], :2], A["rigid_state"][i, fe[1], :2] = c + 0.5 * d * u, c - 0.5 * d * u
            d, u, c = kw.pop("knee_d"), np.array([-0.8, 0.6]), np.array([-0.05, 0.21])
            A["rigid_state"][i, kn[0], :2], A["rigid_state"][i, kn[1], :2] = c + 0.5 * d * u, c - 0.5 * d * u
        if "yaw_roll" in kw:
            tot, side = kw.pop("yaw_roll")
            y = L.yaw_roll
            lft, rgt = (tot * 0.6, tot * 0.4) if side == "both" else ((tot, 0.0) if side == "left" else (0.0, tot))
            A["dof_pos"][i, [y[0], y[1]]] = cfg.default[[y[0], y[1]]] + lft * np.array([0.6, -0.8])
            A["dof_pos"][i, [y[2], y[3]]] = cfg.default[[y[2], y[3]]] + rgt * np.array([-0.8, 0.6])
        if "jp_norm" in kw:  # ref = q - direction x norm
            d = _unit(r.uniform(-1, 1, 12))
            A["ref_dof_pos"][i] = A["dof_pos"][i].astype(f64) - d * kw.pop("jp_norm")
        for key, arr in (("vb", vb), ("wb", wb), ("lrv_delta", lrv_delta), ("rpy", rpy)):
            if key in kw:
                arr[i] = kw.pop(key)
        if "bh_arg" in kw:
            bh_arg[i] = kw.pop("bh_arg")
        if kw.pop("sums", False):
            for nm in NAMES:
                A["episode_sums"][nm][i] = f32(sums_rng.rand() - 0.3)
        assert not kw, kw
    # root orientation, then the world-frame velocities that give the planted base-frame ones
    q = np.stack([quat_rpy(*rpy[i]) for i in range(n)])
    A["root_states"][:, 3:7] = q
    q32 = A["root_states"][:, 3:7]
    A["root_states"][:, 7:10] = _apply64(q32, vb)
    A["root_states"][:, 10:13] = _apply64(q32, wb)
    A["last_root_vel"] = (A["root_states"][:, 7:13].astype(f64) + lrv_delta).astype(f32)
    # root z from the base_height argument: z - (stance-weighted foot height - 0.05) - target
    _, _, st = E.gait(A["episode_length_buf"].astype(np.int64) + 1, cfg.P)
    mh = (A["rigid_state"][:, fe, 2].astype(f64) * st).sum(1) / st.sum(1)
    A["root_states"][:, 2] = float(f32(cfg.P.base_height_target)) + (mh - float(f32(0.05))) + bh_arg
    # frame entries beyond the clip (exactly +-clip in both tables) and their partners inside
    clip = float(cfg.c.clip_observations)
    os_ = cfg.P.obs_scales
    for i in tb.groups["clip"]:
        kw = tb.rows[i]

        def mark(val, cols):
            for t, c in cols:
                if abs(val) >= clip:
                    tb.clip.append((i, t, c, 1.0 if val > 0 else -1.0))
                elif abs(val) > 0.9 * clip:
                    tb.inside.append((i, t, c))
        for j, v in kw.get("qd", {}).items():
            mark(v * os_["dof_vel"], [("o", 17 + j), ("p", 17 + j)])
        for j, v in kw.get("act", {}).items():
            mark(v, [("o", 29 + j), ("p", 29 + j)])
        for j, v in kw.get("q", {}).items():
            mark((v - cfg.default[j]) * os_["dof_pos"], [("o", 5 + j), ("p", 5 + j), ("p", 41 + j)])
        for a, v in enumerate(kw.get("wb", ())):
            mark(v * os_["ang_vel"], [("o", 41 + a), ("p", 56 + a)])
        for a, v in enumerate(kw.get("vb", ())):
            mark(v * os_["lin_vel"], [("p", 53 + a)])
        for a, v in enumerate(kw.get("pf", ())):
            mark(v, [("p", 62 + a)])
        for a, v in enumerate(kw.get("pt", ())):
            mark(v, [("p", 64 + a)])
        if "fric" in kw:
            mark(kw["fric"], [("p", 67)])
            mark(kw["mass"] / 30.0, [("p", 68)])
    tb.resample = np.nonzero((A["episode_length_buf"].astype(np.int64) + 1) % int(cfg.c.resample_interval) == 0)[0]
    return A, tb


# ------------------------------------------------------------------------------------------ reference
def derived64(S, cfg):
    """The state envlogic_ref.rewards reads, as pipeline_ref.post derives it before the rewards, in
    float64 from the float32 snapshot (no resample: the resample rows are excluded from the
    command-dependent comparisons).  Also the absolute error bounds of the derived quantities a
    float32 evaluation may carry: `err` name -> [N] or [N, k]."""
    D = {k: (copy.deepcopy(v) if isinstance(v, dict) else np.array(v)) for k, v in S.items()}
    n = D["root_states"].shape[0]
    q = S["root_states"][:, 3:7]
    D["episode_length_buf"] = S["episode_length_buf"].astype(np.int64) + 1
    v, w = S["root_states"][:, 7:10].astype(f64), S["root_states"][:, 10:13].astype(f64)
    D["base_lin_vel"], D["base_ang_vel"] = _rot_inv64(q, v), _rot_inv64(q, w)
    g = np.tile(np.array([0.0, 0.0, -1.0]), (n, 1))
    D["projected_gravity"] = _rot_inv64(q, g)
    D["base_euler_xyz"] = _euler64(q)
    fwd = _apply64(q, np.tile(np.array([1.0, 0.0, 0.0]), (n, 1)))
    heading = np.arctan2(fwd[:, 1], fwd[:, 0])
    cmd = S["commands"].astype(f64)
    cmd[:, 2] = np.clip(0.5 * _wrap64(cmd[:, 3] - heading), -1.0, 1.0)
    D["commands"] = cmd
    D["default_dof_pos"] = np.broadcast_to(cfg.default[None, :], (n, 12)).astype(f64)
    for k in ("dof_pos", "dof_vel", "actions", "last_actions", "last_last_actions", "contact_forces", "rigid_state",
              "root_states", "last_root_vel", "last_dof_vel", "feet_air_time", "feet_height", "last_feet_z", "ref_dof_pos",
              "torques"):
        D[k] = np.asarray(S[k]).astype(f64)
    # a rotation of v by a unit quaternion: 8 roundings on products that sum to at most 3 |v|
    rot = lambda x: 8 * U * 3 * np.linalg.norm(x, axis=1, keepdims=True) * np.ones((1, 3))  # noqa: E731
    qx, qy, qz, qw = [q[:, i].astype(f64) for i in range(4)]
    # atan2(s, c): (ds + dc) / hypot(s, c) + 4 ulp of the angle; asin(s): ds / sqrt(1 - s^2) + 4 ulp;
    # the wrap adds and removes 2 pi for negative angles: two roundings at magnitude 2 pi (2^-21)
    wrap = 2.0 ** -21
    e_c = 5 * U
    sr, cr = 2 * (qw * qx + qy * qz), qw * qw - qx * qx - qy * qy + qz * qz
    e_roll = (6 * U * (abs(qw * qx) + abs(qy * qz)) + e_c) / np.hypot(sr, cr) + 8 * U * abs(D["base_euler_xyz"][:, 0]) + wrap
    sp = 2 * (qw * qy - qz * qx)
    e_pitch = 6 * U * (abs(qw * qy) + abs(qz * qx)) / np.sqrt(np.maximum(1 - sp * sp, 1e-6)) + 8 * U * abs(D["base_euler_xyz"][:, 1]) + wrap
    e_head = 2 * rot(np.ones((n, 1)))[:, 0] / np.hypot(fwd[:, 0], fwd[:, 1]) + 8 * U * abs(heading)
    e_cmd2 = 0.5 * (e_head + U * (abs(cmd[:, 3]) + abs(heading)) + wrap)
    err = dict(blv=rot(v), bav=rot(w), pg=rot(g), roll=e_roll, pitch=e_pitch, cmd2=e_cmd2)
    return D, err


def _exp_err(arg, arg_err):
    return np.exp(-arg) * (arg_err + (np.abs(arg) + 2) * 2.0 ** -23)


def _sqrt_err(x, x_err):
    s = np.sqrt(x)
    return np.minimum(x_err / np.maximum(2 * s, 1e-300), np.sqrt(x_err)) + U * s


def term_bounds(D, err, cfg):
    """Absolute bound of a float32 evaluation of each continuous term against exact arithmetic on the
    same float32 inputs: name -> [N].  D, err: derived64's."""
    P, L = cfg.P, cfg.L
    fe, kn = list(L.feet), list(L.knees)
    a, la, lla = np.abs(D["actions"]), np.abs(D["last_actions"]), np.abs(D["last_last_actions"])
    B = {}
    # d = la - a (1), square (1), 12 adds; second difference: 2 adds; sum |a|: 12 adds, x 0.05, 2 adds
    m1, m2, m3 = ((la + a) ** 2).sum(1), ((a + lla + 2 * la) ** 2).sum(1), a.sum(1)
    B["action_smoothness"] = 15 * U * m1 + 17 * U * m2 + 14 * U * 0.05 * m3 + 2 * U * (m1 + m2 + 0.05 * m3)
    # base_acc: 6 differences (1), squares (1), 6 adds, sqrt, x 3, exp
    lrv, rv = D["last_root_vel"], D["root_states"][:, 7:13]
    ss = ((lrv - rv) ** 2).sum(1)
    e_n = _sqrt_err(ss, 9 * U * ((np.abs(lrv) + np.abs(rv)) ** 2).sum(1))
    B["base_acc"] = _exp_err(3 * np.sqrt(ss), 3 * e_n + U * 3 * np.sqrt(ss))
    # base_height: weighted mean (1 add, 1 divide), - 0.05, z - (.), - target, abs, x 100
    _, _, st = E.gait(D["episode_length_buf"], P)
    fzr = D["rigid_state"][:, fe, 2]
    mh = (fzr * st).sum(1) / st.sum(1)
    inner = D["root_states"][:, 2] - (mh - float(f32(0.05))) - float(f32(P.base_height_target))
    mag = np.abs(D["root_states"][:, 2]) + np.abs(fzr).sum(1) + 0.05 + float(P.base_height_target)
    B["base_height"] = _exp_err(100 * np.abs(inner), 100 * 5 * U * mag + U * 100 * np.abs(inner))
    # default_joint_pos: two 2-norms (4 roundings on the squares' sum, sqrt), add, - 0.1, clamp, x 100,
    # exp; 0.01 x 12-norm; subtract
    jd = D["dof_pos"] - D["default_dof_pos"]
    y = L.yaw_roll
    lft, rgt = np.hypot(jd[:, y[0]], jd[:, y[1]]), np.hypot(jd[:, y[2]], jd[:, y[3]])
    yv = np.clip(lft + rgt - float(f32(0.1)), 0, 50)
    e_y = 5 * U * (lft + rgt + 0.1)
    ex = np.exp(-100 * yv)
    nj = np.linalg.norm(jd, axis=1)
    B["default_joint_pos"] = _exp_err(100 * yv, 100 * e_y + U * 100 * yv) + 10 * U * 0.01 * nj + U * (ex + 0.01 * nj)
    # dof_acc: difference (1), / dt (1), square (1), 12 adds; dof_vel, torques: square, 12 adds
    B["dof_acc"] = 17 * U * (((np.abs(D["last_dof_vel"]) + np.abs(D["dof_vel"])) / float(f32(P.dt))) ** 2).sum(1)
    B["dof_vel"] = 13 * U * (D["dof_vel"] ** 2).sum(1)
    B["torques"] = 13 * U * (D["torques"] ** 2).sum(1)
    # feet_contact_forces: 3-norm (3 u relative), - max (1), clamps (continuous), 1 add
    nf = np.linalg.norm(D["contact_forces"][:, fe, :], axis=-1)
    B["feet_contact_forces"] = 5 * U * (nf + float(P.max_contact_force)).sum(1)
    # foot_slip: 2-norm (2 u relative), sqrt (+ u / 2 + u), 1 add
    sl = np.sqrt(np.linalg.norm(D["rigid_state"][:, fe, 10:12], axis=2)) * (D["contact_forces"][:, fe, 2] > 5.0)
    B["foot_slip"] = 4 * U * sl.sum(1)

    def dist(pos, mx):
        p0, p1 = pos[:, 0, :], pos[:, 1, :]
        d = np.linalg.norm(p0 - p1, axis=1)
        e_d = U * (np.abs(p0) + np.abs(p1)).sum(1) + 3 * U * d
        tot = 0.0
        for thr, lo_, hi_ in ((float(f32(P.min_dist)), -0.5, 0.0), (float(f32(mx)), 0.0, 0.5)):
            arg = 100 * np.abs(np.clip(d - thr, lo_, hi_))
            tot = tot + _exp_err(arg, 100 * (e_d + U * (d + thr)) + U * arg) / 2
        return tot + 2 * U
    B["feet_distance"] = dist(D["rigid_state"][:, fe, :2], P.max_dist)
    B["knee_distance"] = dist(D["rigid_state"][:, kn, :2], P.max_dist / 2)
    # joint_pos: 12 differences, squares, 12 adds, sqrt; exp(-2 n) - 0.2 clamp(n)
    q, rf = D["dof_pos"], D["ref_dof_pos"]
    s2 = ((q - rf) ** 2).sum(1)
    e_n = _sqrt_err(s2, 15 * U * ((np.abs(q) + np.abs(rf)) ** 2).sum(1))
    nd = np.sqrt(s2)
    B["joint_pos"] = _exp_err(2 * nd, 2 * e_n) + 0.2 * e_n + 2 * U * (np.exp(-2 * nd) + 0.1)
    # orientation: (exp(-10 (|roll| + |pitch|)) + exp(-20 |pg_xy|)) / 2
    eul, pg = D["base_euler_xyz"], D["projected_gravity"]
    a1 = 10 * (np.abs(eul[:, 0]) + np.abs(eul[:, 1]))
    n2 = np.hypot(pg[:, 0], pg[:, 1])
    e_n2 = err["pg"][:, 0] + err["pg"][:, 1] + 3 * U * n2
    B["orientation"] = (_exp_err(a1, 10 * (err["roll"] + err["pitch"]) + 2 * U * a1) + _exp_err(20 * n2, 20 * e_n2 + U * 20 * n2)) / 2 + 2 * U
    # tracking terms
    cmd, blv, bav = D["commands"], D["base_lin_vel"], D["base_ang_vel"]
    ex_, ey_ = cmd[:, 0] - blv[:, 0], cmd[:, 1] - blv[:, 1]
    e_ex = err["blv"][:, 0] + U * (np.abs(cmd[:, 0]) + np.abs(blv[:, 0]))
    e_ey = err["blv"][:, 1] + U * (np.abs(cmd[:, 1]) + np.abs(blv[:, 1]))
    le = np.hypot(ex_, ey_)
    e_le = e_ex + e_ey + 3 * U * le
    ae = cmd[:, 2] - bav[:, 2]
    e_ae = err["cmd2"] + err["bav"][:, 2] + U * (np.abs(cmd[:, 2]) + np.abs(bav[:, 2]))
    B["track_vel_hard"] = ((_exp_err(10 * le, 10 * e_le + U * 10 * le) + _exp_err(10 * np.abs(ae), 10 * e_ae + U * 10 * np.abs(ae))) / 2
                           + 0.2 * (e_le + e_ae) + 4 * U * (1 + 0.2 * (le + np.abs(ae))))
    sg = float(f32(P.tracking_sigma))
    B["tracking_ang_vel"] = _exp_err(sg * ae * ae, sg * 2 * np.abs(ae) * e_ae + 2 * U * sg * ae * ae)
    l2 = ex_ * ex_ + ey_ * ey_
    B["tracking_lin_vel"] = _exp_err(sg * l2, sg * 2 * (np.abs(ex_) * e_ex + np.abs(ey_) * e_ey) + 4 * U * sg * l2)
    nw = np.hypot(bav[:, 0], bav[:, 1])
    e_nw = err["bav"][:, 0] + err["bav"][:, 1] + 3 * U * nw
    bz = blv[:, 2]
    B["vel_mismatch_exp"] = (_exp_err(10 * bz * bz, 20 * np.abs(bz) * err["blv"][:, 2] + 2 * U * 10 * bz * bz)
                             + _exp_err(5 * nw, 5 * e_nw + U * 5 * nw)) / 2 + 2 * U
    return B


def reference(S, hist_o, hist_p, cfg, counter=COUNTER, pipeline=PR):
    """The float32 pipeline on a copy of S and the float64 terms with their bounds.  `pipeline`: the
    pipeline module (a mutated copy in the CPU mutant test)."""
    S32 = copy.deepcopy(S)
    extras = {}
    obs, priv, rew, reset, timeout, terms = pipeline.post(cfg, S32, counter, hist_o, hist_p, extras=extras)
    n = S["root_states"].shape[0]
    ref = dict(S32=S32, extras=extras, obs=obs, priv=priv, rew=rew, reset=np.asarray(reset, bool), timeout=np.asarray(timeout, bool), terms32=terms,
               planted_sums={nm: np.array(S["episode_sums"][nm]) for nm in NAMES})
    ref["inc32"] = {nm: (terms[nm] * f32(cfg.scales[nm])).astype(f32) for nm in NAMES}
    D, err = derived64(S, cfg)
    ref["D"], ref["err"] = D, err
    t64 = E.rewards(copy.deepcopy(D), cfg.L, cfg.P, f64)
    sums64 = {nm: np.zeros(n, f64) for nm in NAMES}
    ref["total64"] = E.total_reward(t64, cfg.scales, sums64, cfg.P, f64)
    ref["terms64"], ref["inc64"] = t64, sums64
    ref["raw_total64"] = sum(sums64[nm] for nm in NAMES)
    tbnd = term_bounds(D, err, cfg)
    # the scaled increment: the term's bound x |scale| and one rounding of the product
    ref["bound"] = {nm: (tbnd[nm] * abs(cfg.scales[nm]) + U * np.abs(sums64[nm])) if nm in tbnd else np.zeros(n) for nm in NAMES}
    # the total: the increments' bounds and at most 22 + 8 additions on partial sums below sum |r_k|
    ref["total_bound"] = sum(ref["bound"][nm] for nm in NAMES) + 30 * U * sum(np.abs(sums64[nm]) for nm in NAMES)
    return ref


def collect(S_after, obs_stack, priv_stack, rew, reset, timeout):
    """The compared outputs of one post from a state dict after it (the oracle's mutated S, or a
    snapshot of the env) and the returned / published buffers."""
    return dict(reset=np.asarray(reset, bool), timeout=np.asarray(timeout, bool),
                ep=np.asarray(S_after["episode_length_buf"]).astype(np.int64), last_contacts=np.asarray(S_after["last_contacts"], bool),
                sums=np.stack([np.asarray(S_after["episode_sums"][nm], f32) for nm in NAMES]), rew=np.asarray(rew, f32),
                fat=S_after["feet_air_time"], fht=S_after["feet_height"], lfz=S_after["last_feet_z"], commands=S_after["commands"],
                ref_dof_pos=S_after["ref_dof_pos"], obs=np.asarray(obs_stack)[:, -47:], priv=np.asarray(priv_stack)[:, -73:],
                obs_stack=np.asarray(obs_stack), priv_stack=np.asarray(priv_stack))


def check(got, ref, tb, cfg):
    """Every comparison of tests/test_gpu_reward_terms.py.  Returns (violations, worst): a list of
    strings (empty = pass) and, per term and for the total, the largest |got - float64| / bound."""
    bad, worst = [], {}
    S32 = ref["S32"]
    n = len(ref["reset"])
    reset = ref["reset"]
    keep = ~reset
    excl = np.zeros(n, bool)
    excl[tb.resample] = True

    every = np.ones(n, bool)

    def exact(name, a, b, rows=every):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            bad.append(f"{name}: shape {a.shape}, want {b.shape}")
            return
        m = (a != b).reshape(n, -1).any(1) & rows
        if m.any():
            bad.append(f"{name}: differs in rows {np.nonzero(m)[0]}")

    def close(name, a, b, rtol, atol, rows=every):
        a, b = np.asarray(a, f64), np.asarray(b, f64)
        m = (np.abs(a - b) > atol + rtol * np.abs(b)).reshape(n, -1) & rows[:, None]
        if m.any():
            bad.append(f"{name}: {int(m.sum())} entries off, worst {(np.abs(a - b).reshape(n, -1) * m).max():.3g}, rows {np.nonzero(m.any(1))[0]}")

    # flags and discrete state
    exact("reset_buf", got["reset"], reset)
    exact("time_out_buf", got["timeout"], ref["timeout"])
    exact("episode_length_buf", got["ep"], np.asarray(S32["episode_length_buf"]).astype(np.int64))
    exact("last_contacts", got["last_contacts"], S32["last_contacts"])
    exact("stance / contact columns", got["priv"][:, 69:73], ref["priv"][:, -73:][:, 69:73])
    # per-term sums
    for k, nm in enumerate(NAMES):
        s = got["sums"][k]
        if (s[reset] != 0).any():
            bad.append(f"sums[{nm}] not cleared on the resetting rows")
        if nm in DISCRETE:
            rows = keep & ~(excl if nm in CMD_TERMS else np.zeros(n, bool))
            exact(f"sums[{nm}] (bitwise)", s, ref["inc32"][nm], rows)
            continue
        rows = keep & ~(excl if nm in CMD_TERMS else np.zeros(n, bool))
        d = np.abs(s.astype(f64) - ref["inc64"][nm])[rows]
        b = ref["bound"][nm][rows]
        ratio = np.where(b > 0, d / np.where(b > 0, b, 1), np.where(d > 0, np.inf, 0.0))
        worst[nm] = float(ratio.max())
        if (d > b).any():
            w = np.nonzero(rows)[0][d > b]
            bad.append(f"sums[{nm}]: |got - f64| / bound up to {ratio.max():.3g} in rows {w}")
    # the excluded rows still hold the float32 oracle's tolerance of _post_parity
    for k, nm in enumerate(NAMES):
        if nm in CMD_TERMS:
            close(f"sums[{nm}] (resample rows)", got["sums"][k], S32["episode_sums"][nm], 2e-4, 1e-6, excl & keep)
    # total reward
    rows = ~excl
    d = np.abs(got["rew"].astype(f64) - ref["total64"])[rows]
    b = ref["total_bound"][rows]
    worst["total"] = float((d / b).max())
    if (d > b).any():
        bad.append(f"rew_buf: |got - f64| / bound up to {(d / b).max():.3g} in rows {np.nonzero(rows)[0][d > b]}")
    neg = ref["raw_total64"] < -10 * ref["total_bound"]
    if (got["rew"][neg & rows] != 0).any():
        bad.append("rew_buf: a clearly negative total is not exactly 0")
    close("rew_buf (resample rows)", got["rew"], ref["rew"], 2e-4, 2e-5, excl)
    # carried state: single float32 operations (fat + dt; fz - 0.05; fht + (fz - lfz), no product to fuse)
    exact("feet_air_time", got["fat"], S32["feet_air_time"])
    exact("last_feet_z", got["lfz"], S32["last_feet_z"])
    exact("feet_height", got["fht"], S32["feet_height"])
    close("commands", got["commands"], S32["commands"], 1e-5, 1e-5)
    plain = keep & ~excl
    exact("commands[:, (0, 1, 3)] of the rows that neither reset nor resample", got["commands"][:, [0, 1, 3]], S32["commands"][:, [0, 1, 3]], plain)
    d = np.abs(got["commands"][:, 2].astype(f64) - ref["D"]["commands"][:, 2])[plain]
    b = ref["err"]["cmd2"][plain] + U
    worst["commands[2]"] = float((d / b).max())
    if (d > b).any():
        bad.append(f"commands[:, 2]: |got - f64| / bound up to {(d / b).max():.3g}")
    # ref_dof_pos: sin x scale, 2 ulp of the sine and one product; exact zeros inside the window
    close("ref_dof_pos", got["ref_dof_pos"], S32["ref_dof_pos"], 0, 6 * U * 2 * cfg.P.target_joint_pos_scale)
    exact("ref_dof_pos zeros", np.asarray(got["ref_dof_pos"]) == 0, np.asarray(S32["ref_dof_pos"]) == 0)
    # observation frames
    clip = f32(cfg.c.clip_observations)
    fr = {"o": got["obs"], "p": got["priv"]}
    for i, t, c, sgn in tb.clip:
        if fr[t][i, c] != f32(sgn) * clip:
            bad.append(f"frame {t}[{i}, {c}] = {fr[t][i, c]!r}, planted beyond the clip: want {sgn * clip}")
    for i, t, c in tb.inside:
        if not abs(fr[t][i, c]) < clip:
            bad.append(f"frame {t}[{i}, {c}] = {fr[t][i, c]!r}, planted inside the clip")
    close("obs_buf", got["obs_stack"], ref["obs"], 1e-4, 1e-4)
    close("privileged_obs_buf", got["priv_stack"], ref["priv"], 1e-4, 1e-4)
    return bad, worst


# ------------------------------------------------------------------------------------------ coverage
def branches(S, ref, tb, cfg):
    """(branch list, margin list) of the planted table.  Branch: (name, bool [N], reset_allowed):
    both values must occur in at least 2 rows (rows that do not reset unless reset_allowed: the
    termination itself).  Margin: (name, quantity [N] or [N, 2], threshold, relative margin): the
    float32 quantity must stay that far from the threshold in every row."""
    P, L, D = cfg.P, cfg.L, ref["D"]
    fe, kn = list(L.feet), list(L.knees)
    ep1 = D["episode_length_buf"]
    s, _, st = E.gait(ep1, P)
    cf = S["contact_forces"].astype(f32)
    bn = np.linalg.norm(cf[:, L.base, :], axis=-1)
    fz = cf[:, fe, 2]
    con = fz > 5.0
    fn = np.linalg.norm(cf[:, fe, :], axis=-1)
    Br, Mg = [], []
    Br += [("base force > 1", bn > 1.0, True), ("ep > max", ep1 > P.max_episode_length, True), ("base force > 0.1", bn > 0.1, False)]
    Mg += [("base force vs 1", bn, 1.0, MARGIN), ("base force vs 0.1", bn, 0.1, MARGIN)]
    Br += [("sin >= 0", s >= 0, False), ("|sin| < 0.1", np.abs(s) < 0.1, False)]
    Mg += [("|sin| vs 0.1", np.abs(s), 0.1, 1e-2)]
    for f in range(2):
        Br += [(f"contact foot {f}", con[:, f], False), (f"contact == stance foot {f}, stance", con[:, f][st[:, f] == 1], False),
               (f"contact == stance foot {f}, swing", con[:, f][st[:, f] == 0], False),
               (f"foot force {f} > max", fn[:, f] > P.max_contact_force, False), (f"foot force {f} > max + 400", fn[:, f] > P.max_contact_force + 400, False)]
    Mg += [("fz vs 5", fz, 5.0, MARGIN), ("foot force vs max", fn, P.max_contact_force, MARGIN), ("foot force vs max + 400", fn, P.max_contact_force + 400, MARGIN)]
    fat = S["feet_air_time"].astype(f32)
    filt = con | (st != 0) | np.asarray(S["last_contacts"], bool)
    fh = S["feet_height"].astype(f32) + ((S["rigid_state"][:, fe, 2].astype(f32) - f32(0.05)) - S["last_feet_z"].astype(f32))
    dev = np.abs(fh - f32(P.target_feet_height))
    for f in range(2):
        Br += [(f"air time > 0 foot {f}", fat[:, f] > 0, False), (f"filter foot {f}", filt[:, f], False),
               (f"first contact foot {f}", (fat[:, f] > 0) & filt[:, f], False), (f"air time + dt > 0.5 foot {f}", fat[:, f] + f32(P.dt) > 0.5, False),
               (f"last_contacts only foot {f}", (S["last_contacts"][:, f] & ~con[:, f] & (st[:, f] == 0))[fat[:, f] > 0], False),
               (f"clearance foot {f}, swing", (dev[:, f] < 0.01)[st[:, f] == 0], False), (f"clearance foot {f}, stance", (dev[:, f] < 0.01)[st[:, f] == 1], False),
               (f"clearance foot {f}, contact", (dev[:, f] < 0.01)[con[:, f]], False)]
    Mg += [("air time + dt vs 0.5", fat + f32(P.dt), 0.5, MARGIN), ("|feet height - target| vs 0.01", dev, 0.01, MARGIN)]
    for nm, bodies, mx in (("feet", fe, P.max_dist), ("knee", kn, P.max_dist / 2)):
        p = S["rigid_state"][:, bodies, :2].astype(f32)
        d = np.linalg.norm(p[:, 0] - p[:, 1], axis=1)
        Br += [(f"{nm} distance < min", d < P.min_dist, False), (f"{nm} distance > max", d > mx, False), (f"{nm} distance > max + 0.5", d > mx + 0.5, False)]
        Mg += [(f"{nm} distance vs min", d, P.min_dist, MARGIN), (f"{nm} distance vs max", d, mx, MARGIN), (f"{nm} distance vs max + 0.5", d, mx + 0.5, MARGIN)]
    jd = S["dof_pos"].astype(f32) - cfg.default[None, :]
    y = L.yaw_roll
    lft, rgt = np.hypot(jd[:, y[0]], jd[:, y[1]]), np.hypot(jd[:, y[2]], jd[:, y[3]])
    nd = np.linalg.norm(S["dof_pos"].astype(f32) - S["ref_dof_pos"].astype(f32), axis=1)
    Br += [("yaw / roll sum > 0.1", lft + rgt > 0.1, False), ("yaw / roll sum > 0.1, left pair alone", (lft > 0.1)[rgt == 0], False),
           ("yaw / roll sum > 0.1, right pair alone", (rgt > 0.1)[lft == 0], False), ("|q - ref| > 0.5", nd > 0.5, False)]
    Mg += [("yaw / roll sum vs 0.1", lft + rgt, 0.1, MARGIN), ("|q - ref| vs 0.5", nd, 0.5, MARGIN)]
    blx, cx = D["base_lin_vel"][:, 0].astype(f32), S["commands"][:, 0].astype(f32)
    sp, cm = np.abs(blx), np.abs(cx)
    live = ~np.isin(np.arange(len(cx)), tb.resample)
    Br += [("speed < 0.5 cmd", (sp < 0.5 * cm)[live], False), ("speed > 1.2 cmd", (sp > 1.2 * cm)[live], False),
           ("desired speed", ~((sp < 0.5 * cm) | (sp > 1.2 * cm))[live & (np.sign(blx) == np.sign(cx))], False),
           ("sign mismatch", (np.sign(blx) != np.sign(cx))[live], False), ("|cmd| > 0.1", (cm > 0.1)[live], False),
           ("desired speed at gated command", (cm > 0.1)[live & (np.sign(blx) == np.sign(cx)) & (sp > 0.5 * cm) & (sp < 1.2 * cm)], False)]
    nz = cm > 0
    Mg += [("speed vs 0.5 cmd", np.where(nz, sp / np.where(nz, cm, 1), 9.0), 0.5, MARGIN), ("speed vs 1.2 cmd", np.where(nz, sp / np.where(nz, cm, 1), 9.0), 1.2, MARGIN),
           ("|cmd| vs 0.1", cm, 0.1, MARGIN)]
    fwd = _apply64(S["root_states"][:, 3:7], np.tile(np.array([1.0, 0.0, 0.0]), (len(cx), 1)))
    hw = 0.5 * _wrap64(S["commands"][:, 3].astype(f64) - np.arctan2(fwd[:, 1], fwd[:, 0]))
    Br += [("heading command > 1", (hw > 1)[live], False), ("heading command < -1", (hw < -1)[live], False)]
    Mg += [("|heading command| vs 1", np.abs(hw), 1.0, MARGIN), ("wrapped heading vs pi", np.abs(2 * hw), np.pi, MARGIN)]
    Br += [("total < 0", (ref["raw_total64"] < 0)[live], False), ("resample", ~live, False)]
    return Br, Mg
