"""Stride statistics: a float64 statement of the stride detector's sample rule, its ground-height rule
and both fold modes (include/hgsim.h, "stride statistics"), written from the specification and not
from the kernel's header.  TEST INFRASTRUCTURE: tests/test_stride_cases.py runs the host build of the
kernel's sample function against it, tests/test_gpu_stride.py the kernels.

State layout: the env's views, env-major: root_states [n, 13], contact_forces [n, 13, 3],
rigid_state [n, 13, 13]; a sequence adds a leading [T].  Detector state [16, n] and accumulators
run / done [20, n] float64, foot-major (row f * slots + k).  A terrain is None (plane) or a dict
hf (int16 [rows, cols]), hs, vs, border (float32 scalars).

Every env is advanced by plain float64 scalar arithmetic in the order the specification writes, so
the kernel and this file differ only by the rounding of sqrt and divide.
"""
import numpy as np

import metrics_ref as MR

NAMES = ["strides", "swing_time", "clearance", "step_length", "step_width", "touchdown_force", "stride_pairs",
         "stride_length", "stride_time", "short_swings"]
STATE_NAMES = ["phase", "phase_steps", "since_td", "has_anchor", "anchor_x", "anchor_y", "ref_hag", "apex_hag"]
STATE_KEYS = ["root_states", "contact_forces", "rigid_state"]
NS, NST = len(NAMES), len(STATE_NAMES)
CONTACT_Z = MR.CONTACT_Z
FEET = MR.FEET
MIN_SWING = 3
COUNT_SLOTS = [NAMES.index(k) for k in ("strides", "stride_pairs", "short_swings")]   # integer-valued sums
SUM_SLOTS = [k for k in range(NS) if k not in COUNT_SLOTS]
F64 = np.float64


def ground(x, y, terrain):
    """h(x, y): 0 on a plane, else vs * min(hf[i][j], hf[i+1][j], hf[i][j+1]) with (i, j) =
    (p + border) / hs truncated and clipped to [0, rows-2] x [0, cols-2]."""
    if terrain is None:
        return F64(0.0)
    hf = np.asarray(terrain["hf"])
    rows, cols = hf.shape
    hs, vs, border = (F64(np.float32(terrain[k])) for k in ("hs", "vs", "border"))
    i = int(min(max(np.trunc((F64(x) + border) / hs), 0), rows - 2))
    j = int(min(max(np.trunc((F64(y) + border) / hs), 0), cols - 2))
    return vs * F64(min(int(hf[i, j]), int(hf[i + 1, j]), int(hf[i, j + 1])))


def _advance_env(q, fz, p, terrain, dt, st, run):
    """One sample of one env in place: q [4], fz [2], p [2, 3] float64; st [2, 8], run [2, 10]."""
    read = np.concatenate([q, fz, p.reshape(-1)])
    ok = bool(np.isfinite(read).all())
    if ok:
        with np.errstate(all="ignore"):
            qn = F64(1.0) / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
            qx, qy, qz, qw = q[0] * qn, q[1] * qn, q[2] * qn, q[3] * qn
            fx = 1.0 - 2.0 * (qy * qy + qz * qz)
            fy = 2.0 * (qx * qy + qz * qw)
            nrm = np.sqrt(fx * fx + fy * fy)
            ok = bool(nrm > 0)
    if not ok:
        st[:] = 0.0
        return False
    hx, hy = fx / nrm, fy / nrm
    hag = [p[f, 2] - ground(p[f, 0], p[f, 1], terrain) for f in range(2)]
    PH, STEPS, SINCE, HAS, AX, AY, REF, APEX = range(8)
    for f in range(2):
        s, r = st[f], run[f]
        contact = bool(fz[f] > CONTACT_Z)
        phase = int(s[PH])
        if phase == 0:
            s[PH], s[STEPS] = (1.0 if contact else 3.0), 1.0
            s[REF if contact else APEX] = hag[f]
        elif phase == 1 and contact:
            s[STEPS] += 1.0
            s[REF] = hag[f]
            s[SINCE] += s[HAS]
        elif phase == 1:
            s[PH], s[STEPS], s[APEX] = 2.0, 1.0, hag[f]
            s[SINCE] += s[HAS]
        elif not contact:
            s[STEPS] += 1.0
            s[APEX] = max(s[APEX], hag[f])
            s[SINCE] += s[HAS]
        elif phase == 2:
            s[SINCE] += s[HAS]
            if s[STEPS] < MIN_SWING:
                r[NAMES.index("short_swings")] += 1.0
            else:
                o = 1 - f
                rx, ry = p[f, 0] - p[o, 0], p[f, 1] - p[o, 1]
                along = rx * hx + ry * hy
                lat = ry * hx - rx * hy
                r[0] += 1.0
                r[1] += s[STEPS] * dt
                r[2] += s[APEX] - s[REF]
                r[3] += along
                r[4] += abs(lat)
                r[5] += fz[f]
                if s[HAS] != 0:
                    dx, dy = p[f, 0] - s[AX], p[f, 1] - s[AY]
                    r[6] += 1.0
                    r[7] += np.sqrt(dx * dx + dy * dy)
                    r[8] += s[SINCE] * dt
                s[AX], s[AY], s[HAS], s[SINCE] = p[f, 0], p[f, 1], 1.0, 0.0
            s[PH], s[STEPS], s[REF] = 1.0, 1.0, hag[f]
        else:
            assert phase == 3
            s[AX], s[AY], s[HAS], s[SINCE] = p[f, 0], p[f, 1], 1.0, 0.0
            s[PH], s[STEPS], s[REF] = 1.0, 1.0, hag[f]
    return True


def sample(state, terrain, dt, st, run, feet=FEET):
    """One stride sample on copies of st [16, n] / run [20, n]: returns (st, run, ok [n] bool)."""
    st, run = np.array(st, F64), np.array(run, F64)
    root = np.asarray(state["root_states"]).astype(F64)
    cf = np.asarray(state["contact_forces"]).astype(F64)
    rg = np.asarray(state["rigid_state"]).astype(F64)
    n = root.shape[0]
    ok = np.zeros(n, bool)
    for e in range(n):
        s, r = st[:, e].reshape(2, NST).copy(), run[:, e].reshape(2, NS).copy()
        fz = np.array([cf[e, b, 2] for b in feet])
        p = np.stack([rg[e, b, 0:3] for b in feet])
        ok[e] = _advance_env(root[e, 3:7], fz, p, terrain, F64(dt), s, r)
        st[:, e], run[:, e] = s.reshape(-1), r.reshape(-1)
    return st, run, ok


def fold(st, run, done, mode, reset=None, mask=None):
    """One stride fold on copies: returns (st, run, done)."""
    st, run, done = np.array(st, F64), np.array(run, F64), np.array(done, F64)
    n = run.shape[1]
    if mode == 1:
        sel = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    else:
        assert mode == 0
        sel = np.asarray(reset).astype(bool)
        done[:, sel] += run[:, sel]
    run[:, sel] = 0.0
    st[:, sel] = 0.0
    return st, run, done


def replay(seq, terrain, dt, st=None, run=None, feet=FEET):
    """Every sample of a [T, n, ...] sequence in order, no folds: returns (st, run, ok [T, n])."""
    T, n = np.asarray(seq["root_states"]).shape[:2]
    st = np.zeros((2 * NST, n)) if st is None else st
    run = np.zeros((2 * NS, n)) if run is None else run
    oks = np.zeros((T, n), bool)
    for t in range(T):
        st, run, oks[t] = sample({k: seq[k][t] for k in STATE_KEYS}, terrain, dt, st, run, feet)
    return st, run, oks


def slot(run, foot, name):
    """Row `name` of foot `foot` of a [20, n] accumulator array."""
    return np.asarray(run)[foot * NS + NAMES.index(name)]


def state_slot(st, foot, name):
    return np.asarray(st)[foot * NST + STATE_NAMES.index(name)]


def compare(got_st, got_run, ref_st, ref_run):
    """The comparison every test applies to every case: counts and state slots exactly (the anchor,
    ref_hag and the max-built apex_hag are copies or differences of inputs: exact too), sums within
    metrics_ref.RTOL / ATOL.  Returns the largest deviation of the sums as a multiple of the bound."""
    np.testing.assert_array_equal(np.asarray(got_st), np.asarray(ref_st))
    got_run, ref_run = np.asarray(got_run, F64), np.asarray(ref_run, F64)
    for f in range(2):
        for k in COUNT_SLOTS:
            np.testing.assert_array_equal(got_run[f * NS + k], ref_run[f * NS + k])
    rows = [f * NS + k for f in range(2) for k in SUM_SLOTS]
    return MR.max_deviation(got_run[rows], ref_run[rows])
