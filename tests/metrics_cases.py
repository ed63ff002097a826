"""Planted states for the gait-metrics sample (hg_metrics_sample, include/hgsim.h).  TEST
INFRASTRUCTURE shared by tests/test_metrics_cases.py (the host build of the sample function) and
tests/test_gpu_metrics.py (the kernel): a table of single-env rows, each aimed at one rule of the
slot table, and helpers that stack rows into env-major float32 state arrays.

Every value is float32 (what the arena holds); the expectation is tests/metrics_ref.py at exactly
these values.
"""
import numpy as np

import metrics_ref as MR

f32 = np.float32
FEET = MR.FEET
# effort x safety.torque_limit of the XBot-L leg joints is not needed here: any positive limits do;
# these are distinct per joint so that a limit read at the wrong index shows
TORQUE_LIMIT = np.array([170.0, 85.0, 85.0, 255.0, 42.5, 21.25, 170.5, 85.5, 85.25, 255.5, 42.75, 21.5], f32)
SIM_DT, DECIMATION = f32(0.001), 10
DT = float(SIM_DT) * DECIMATION          # (double)sim_dt * decimation


def _quat(axis, angle, scale=1.0):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return (scale * np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])).astype(f32)


def base_row(seed=0):
    """A walking-like state: tilted and yawed base, one foot down and sliding, mixed joint powers."""
    rs = np.random.RandomState(100 + seed)
    root = np.zeros(13, f32)
    root[0:3] = (3.0, -2.0, 0.9)
    root[3:7] = _quat((0.2, -0.3, 1.0), 0.7)
    root[7:10] = (0.42, 0.11, -0.03)
    root[10:13] = (0.1, -0.2, 0.33)
    contact = rs.uniform(-1, 1, (13, 3)).astype(f32)
    contact[FEET[0], 2], contact[FEET[1], 2] = 312.5, 0.25
    rigid = rs.uniform(-1, 1, (13, 13)).astype(f32)
    rigid[FEET[0], 7:9] = (0.03, -0.04)
    rigid[FEET[1], 7:9] = (0.6, 0.2)
    return dict(root_states=root, commands=np.array([0.5, -0.1, 0.2, 0.7], f32),
                torques=rs.uniform(-60, 60, 12).astype(f32), dof_vel=rs.uniform(-4, 4, 12).astype(f32),
                contact_forces=contact, rigid_state=rigid, actions=rs.uniform(-1, 1, 12).astype(f32),
                last_actions=rs.uniform(-1, 1, 12).astype(f32))


def _row(name, seed=0, **edit):
    r = base_row(seed)
    for k, fn in edit.items():
        fn(r[k])
    return name, r


def _set(idx, val):
    def fn(a):
        a[idx] = val
    return fn


def _nan_rows():
    """A NaN in each input array in turn, at an element the sample reads; an inf; and NaNs at elements
    it does not read (root position, commands[3], a foot's contact x, a non-foot body), which must not skip."""
    where = {"root_states": 5, "commands": 2, "torques": 7, "dof_vel": 0, "contact_forces": (FEET[1], 2),
             "rigid_state": (FEET[0], 8), "actions": 11, "last_actions": 3}
    rows = [_row("nan_" + k, 20 + i, **{k: _set(idx, np.nan)}) for i, (k, idx) in enumerate(where.items())]
    rows.append(_row("inf_root_vel", 30, root_states=_set(8, np.inf)))
    rows.append(_row("neg_inf_torque", 31, torques=_set(2, -np.inf)))
    return rows


def _unread(r):
    r["root_states"][1] = np.nan
    r["commands"][3] = np.nan
    r["contact_forces"][FEET[0], 0] = np.nan
    r["contact_forces"][3, 2] = np.nan
    r["rigid_state"][FEET[0], 0] = np.nan
    r["rigid_state"][2, 7] = np.nan
    return r


def _mixed_power(r):
    r["torques"][:] = np.array([10, -10, 10, 20, -30, 5, 0, 2, -2, 7, 1, -1], f32)
    r["dof_vel"][:] = np.array([1, 1, 2, 0.5, 1, -1, 3, 1, 1, 1, -2, -2], f32)


def _zero_vel(r):
    r["root_states"][7:13] = 0
    r["dof_vel"][:] = 0
    r["rigid_state"][:, 7:13] = 0


def _at_limit(r):
    r["torques"][:] = (0.5 * TORQUE_LIMIT * np.array([1, -1] * 6, f32)).astype(f32)
    r["torques"][4] = -TORQUE_LIMIT[4]


def build_rows():
    rows = [
        _row("walking", 0),
        _row("quat_unnormalised", 1, root_states=_set(slice(3, 7), _quat((0.2, -0.3, 1.0), 0.7, scale=3.7))),
        _row("rolled_90", 2, root_states=_set(slice(3, 7), _quat((1, 0, 0), np.pi / 2))),
        _row("pitched_yawed", 3, root_states=_set(slice(3, 7), _quat((0.1, 1.0, 0.4), 2.1))),
        ("mixed_power", base_row(4)),
        _row("force_5_and_next", 5, contact_forces=lambda a: (a.__setitem__((FEET[0], 2), f32(5.0)),
                                                              a.__setitem__((FEET[1], 2), np.nextafter(f32(5.0), f32(np.inf))))),
        ("torque_at_limit", base_row(6)),
        ("zero_velocities", base_row(7)),
        _row("double_support", 8, contact_forces=lambda a: (a.__setitem__((FEET[0], 2), 250.0),
                                                            a.__setitem__((FEET[1], 2), 260.0))),
        _row("flight", 9, contact_forces=lambda a: (a.__setitem__((FEET[0], 2), -3.0), a.__setitem__((FEET[1], 2), 0.0))),
        ("nan_where_not_read", _unread(base_row(10))),
    ]
    _mixed_power(rows[4][1])
    _at_limit(rows[6][1])
    _zero_vel(rows[7][1])
    return rows + _nan_rows()


ROWS = build_rows()
NAMES = [n for n, _ in ROWS]
SKIPPED = [n.startswith(("nan_", "inf_", "neg_inf_")) and n != "nan_where_not_read" for n in NAMES]


def stack(indices):
    """Env-major float32 state arrays for the rows with these table indices (one env each)."""
    return {k: np.stack([ROWS[i][1][k] for i in indices]).astype(f32) for k in MR.STATE_KEYS}


def to_soa(state, np_):
    """The arena's SoA layout, row stride np_: root [13, np_], commands [4, np_], joint arrays [12, np_],
    contact [39, np_] (row 3 b + i), rigid [169, np_] (row 13 b + f); padding columns zero."""
    n = state["root_states"].shape[0]
    out = {}
    for k in MR.STATE_KEYS:
        a = state[k].reshape(n, -1).T
        buf = np.zeros((a.shape[0], np_), f32)
        buf[:, :n] = a
        out[k] = buf
    return out
