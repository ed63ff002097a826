"""Planted sequences for the stride detector (include/hgsim.h, "stride statistics").  TEST
INFRASTRUCTURE shared by tests/test_stride_cases.py (the host build of the sample function) and
tests/test_gpu_stride.py (the kernels): single-env sequences of T = 40 samples, each aimed at one
rule, and helpers that stack them into [T, n, ...] float32 state arrays.

Every value is float32 (what the arena holds); the expectation is tests/stride_ref.py at exactly
these values.  A case is (name, sequence, terrain key): "plane", or "field" for the hand-made 6 x 6
heightfield below; every "field" case is also run on the plane.
"""
import numpy as np

import stride_ref as SR

f32 = np.float32
FEET = SR.FEET
T = 40
SIM_DT, DECIMATION = f32(0.001), 10
DT = float(SIM_DT) * DECIMATION          # (double)sim_dt * decimation
ANKLE = 0.05                             # height of the foot body's origin in stance
HALF_WIDTH = 0.15
FORCE = 310.0

# the hand-made heightfield: rows (x) 0..2 are low, rows 3..5 a 0.2 m step, with one lower notch in
# the step so that the minimum of three neighbours is not simply the own cell; it spans
# x, y in [-0.5, 0.75] (border 0.5, 0.25 m cells)
FIELD = dict(hf=np.array([[0, 0, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0],
                          [0, 0, 4, 0, 0, 0],
                          [40, 40, 40, 40, 40, 40],
                          [40, 40, 40, 30, 40, 40],
                          [40, 40, 40, 40, 40, 44]], np.int16),
             hs=f32(0.25), vs=f32(0.005), border=f32(0.5))
TERRAINS = {"plane": None, "field": FIELD}


def quat(axis, angle, scale=1.0):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return (scale * np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])).astype(f32)


def quat_mul(a, b):
    ax, ay, az, aw = (float(v) for v in a)
    bx, by, bz, bw = (float(v) for v in b)
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], f32)


def runs(pattern):
    """'S6 W26 S8' -> [T] bool contact (S stance, W swing)."""
    out = []
    for tok in pattern.split():
        out += [tok[0] == "S"] * int(tok[1:])
    assert len(out) == T, (pattern, len(out))
    return np.array(out, bool)


def gait(contact, q=None, origin=(0.0, 0.0), yaw=0.0, speed=0.6, lift=0.1, ground_z=None, seed=0):
    """A sequence from a contact pattern [T, 2]: a stance foot stays where it is, a swing foot moves
    forward along the heading at 2 * speed and rises by lift * sin over its swing; the base moves at
    speed.  q: the root quaternion (default: yaw about z).  ground_z(x, y): added to the foot height
    (so a foot can follow a step).  Everything the sample does not read is noise."""
    rs = np.random.RandomState(500 + seed)
    q = quat((0, 0, 1), yaw) if q is None else q
    hx, hy = np.cos(yaw), np.sin(yaw)
    root = np.zeros((T, 13), f32)
    cf = rs.uniform(-1, 1, (T, 13, 3)).astype(f32)
    rg = rs.uniform(-1, 1, (T, 13, 13)).astype(f32)
    pos = [np.array([origin[0] - s * HALF_WIDTH * hy, origin[1] + s * HALF_WIDTH * hx]) for s in (1.0, -1.0)]
    for t in range(T):
        root[t, 0:3] = (origin[0] + speed * DT * t * hx, origin[1] + speed * DT * t * hy, 0.9)
        root[t, 3:7] = q
        root[t, 7:13] = rs.uniform(-1, 1, 6)
        for f in range(2):
            z = ANKLE
            if not contact[t, f]:
                a = t
                while a > 0 and not contact[a - 1, f]:
                    a -= 1
                b = t
                while b < T - 1 and not contact[b + 1, f]:
                    b += 1
                pos[f] = pos[f] + 2 * speed * DT * np.array([hx, hy])
                z += lift * np.sin(np.pi * (t - a + 1) / (b - a + 2))
            if ground_z is not None:
                z += ground_z(pos[f][0], pos[f][1])
            rg[t, FEET[f], 0:3] = (pos[f][0], pos[f][1], z)
            cf[t, FEET[f], 2] = FORCE + 3 * f + t if contact[t, f] else 0.5 * (t % 7)
    return dict(root_states=root, contact_forces=cf, rigid_state=rg)


def _pat(p0, p1):
    return np.stack([runs(p0), runs(p1)], axis=1)


WALK = _pat("S6 W26 S8", "S38 W2")                 # swing 26, stance 38: the other foot half a cycle later
QUICK = _pat("S2 W6 S10 W6 S10 W6", "S10 W6 S10 W6 S8")   # period 16: strides pair up within 40 samples


def _edit(seq, fn):
    seq = {k: v.copy() for k, v in seq.items()}
    fn(seq)
    return seq


def _nan_cases():
    """A non-finite value mid-swing (t = 20 or 21 of foot 0's second swing, 18..23) in each array the
    sample reads, and in elements it does not read."""
    out = []
    base = gait(QUICK, seed=3)                         # t = 20: foot 0 swings, foot 1 stands; strides before and after
    for name, key, idx, val in [("nan_root_quat", "root_states", (20, 4), np.nan),
                                ("inf_contact_z", "contact_forces", (20, FEET[1], 2), np.inf),
                                ("nan_contact_z_swing_foot", "contact_forces", (20, FEET[0], 2), np.nan),
                                ("nan_rigid_pos", "rigid_state", (20, FEET[1], 1), np.nan),
                                ("neg_inf_rigid_z", "rigid_state", (21, FEET[0], 2), -np.inf)]:
        def fn(s, key=key, idx=idx, val=val):
            s[key][idx] = val
        out.append((name, _edit(base, fn), "plane"))

    def unread(s):
        s["root_states"][:, 0:3] = np.nan              # the root position and velocities
        s["root_states"][:, 7:13] = np.inf
        s["contact_forces"][:, :, 0:2] = np.nan        # x, y of every body, z of the others
        for b in range(13):
            if b not in FEET:
                s["contact_forces"][:, b, 2] = np.nan
                s["rigid_state"][:, b, :] = np.nan
        s["rigid_state"][:, :, 3:] = np.nan            # orientation and velocities of the feet
    out.append(("nan_where_not_read", _edit(base, unread), "plane"))
    return out


def _threshold():
    """Contact z of exactly 5.0 is no contact, the next float32 above it is: foot 0 'lifts' while its
    force reads 5.0 and 'lands' at nextafter(5)."""
    seq = gait(_pat("S5 W10 S25", "S40"), seed=4)
    c = seq["contact_forces"]
    c[:5, FEET[0], 2] = np.nextafter(f32(5.0), f32(6.0))
    c[5:15, FEET[0], 2] = f32(5.0)
    c[15:, FEET[0], 2] = np.nextafter(f32(5.0), f32(6.0))
    return "force_5_and_next", seq, "plane"


def _step_z(x, y):
    return float(SR.ground(f32(x), f32(y), FIELD))


def build():
    cases = [
        ("clean_walk", gait(WALK), "plane"),
        ("quick_walk", gait(QUICK, seed=1), "plane"),
        ("opens_mid_swing", gait(_pat("W9 S12 W8 S11", "S40"), seed=2), "plane"),
        ("swing_1_2_3", gait(_pat("S4 W1 S5 W2 S5 W3 S20", "S3 W3 S6 W2 S6 W1 S19"), seed=5), "plane"),
        _threshold(),
        ("yaw_90", gait(QUICK, yaw=np.pi / 2, seed=6), "plane"),
        ("yaw_180", gait(QUICK, yaw=np.pi, seed=7), "plane"),
        ("rolled_pitched", gait(QUICK, q=quat_mul(quat((0, 0, 1), 0.6), quat_mul(quat((0, 1, 0), 0.35), quat((1, 0, 0), -0.4))),
                                yaw=0.6, seed=8), "plane"),
        ("quat_scaled_3p7", gait(QUICK, q=quat((0, 0, 1), 0.6, scale=3.7), yaw=0.6, seed=8), "plane"),
        ("quat_zero", gait(QUICK, q=np.zeros(4, f32), seed=9), "plane"),
        ("nose_down", gait(QUICK, q=quat((0, 1, 0), np.pi / 2), seed=10), "plane"),   # no heading: fx = fy = 0
        ("far_180m", gait(QUICK, origin=(180.0, -127.0), yaw=0.3, seed=11), "plane"),
        ("both_land_together", gait(_pat("S3 W8 S9 W8 S12", "S4 W7 S10 W7 S12"), seed=12), "plane"),
        ("flight", gait(_pat("S5 W8 S7 W8 S12", "S5 W8 S7 W8 S12"), seed=13), "plane"),
        ("foot_only_descends", gait(_pat("S5 W10 S25", "S40"), lift=-0.02, seed=14), "plane"),
    ]
    cases += _nan_cases()
    # the field: a foot walks up the step edge (x from 0.1 to beyond 0.25: cell row 2 -> 3), following the
    # ground; a foot far outside the extent is clamped to the last cell
    cases.append(("field_crosses_edge", gait(_pat("S3 W8 S9 W8 S12", "S12 W8 S9 W8 S3"), origin=(0.08, 0.1), speed=1.2,
                                             ground_z=_step_z, seed=15), "field"))
    cases.append(("field_descends_edge", gait(_pat("S3 W8 S9 W8 S12", "S40"), origin=(0.45, 0.1), yaw=np.pi, speed=1.2,
                                              lift=0.01, ground_z=_step_z, seed=16), "field"))
    cases.append(("field_outside_clamped", gait(QUICK, origin=(5.0, -3.0), yaw=0.2, seed=17), "field"))
    return cases


CASES = build()
NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def group(terrain_key):
    """(names, [T, n, ...] sequence) of the cases run on a terrain: the plane takes every case (the
    field's sequences too), the field its own."""
    sel = [c for c in CASES if terrain_key == "plane" or c[2] == terrain_key]
    seq = {k: np.stack([c[1][k] for c in sel], axis=1) for k in SR.STATE_KEYS}
    return [c[0] for c in sel], seq


def to_soa(state, np_):
    """Env-major float32 state of one sample -> the arena's SoA arrays with row stride np_: root
    [13][np_], contact [39][np_], rigid [169][np_].  Padding columns hold a NaN pattern: reading one is a bug."""
    n = state["root_states"].shape[0]
    out = {}
    for k, rows in (("root_states", 13), ("contact_forces", 39), ("rigid_state", 169)):
        a = np.full((rows, np_), np.nan, f32)
        a[:, :n] = np.asarray(state[k], f32).reshape(n, rows).T
        out[k] = a
    return out
