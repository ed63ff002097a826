"""Gait metrics: a float64 numpy statement of the sample table and of both fold modes
(include/hgsim.h, hg_metrics_sample / hg_metrics_fold), written from the specification and not from
the kernel.  TEST INFRASTRUCTURE: tests/test_metrics_cases.py runs the host build of the kernel's
sample function against it, tests/test_gpu_metrics.py the kernels.

State layout: the env's views, env-major: root_states [N, 13], commands [N, 4], torques / dof_vel /
actions / last_actions [N, 12], contact_forces [N, 13, 3], rigid_state [N, 13, 13].  Accumulators:
run / done [13, N] float64, counts [4, N] int (episodes, falls, time_outs, skipped).

Sums over joints and feet are explicit loops in index order (numpy's own reductions sum pairwise),
so the kernel's order is repeated and the two differ only by the rounding of sqrt and divide.
"""
import numpy as np

NAMES = ["steps", "err_vx2", "err_vy2", "err_wz2", "distance", "work_pos", "torque2", "tilt2", "slip",
         "action_rate2", "double_support", "flight", "peak_torque"]
COUNT_NAMES = ["episodes", "falls", "time_outs", "skipped"]
STATE_KEYS = ["root_states", "commands", "torques", "dof_vel", "contact_forces", "rigid_state", "actions", "last_actions"]
CONTACT_Z = 5.0
FEET = (6, 12)

RTOL, ATOL = 1e-12, 1e-15   # the issue's bound for float sums of at most 100 steps


def rotate_inverse(q, v):
    """v [N, 3] rotated by the inverse of the unit quaternion q [N, 4] (xyzw): a - b + c with
    a = v (2 w^2 - 1), b = 2 w (q_v x v), c = 2 (q_v . v) q_v."""
    x, y, z, w = (q[:, i] for i in range(4))
    s = 2.0 * w * w - 1.0
    cx = y * v[:, 2] - z * v[:, 1]
    cy = z * v[:, 0] - x * v[:, 2]
    cz = x * v[:, 1] - y * v[:, 0]
    d = 2.0 * (x * v[:, 0] + y * v[:, 1] + z * v[:, 2])
    w2 = w * 2.0
    return np.stack([v[:, 0] * s - w2 * cx + d * x, v[:, 1] * s - w2 * cy + d * y, v[:, 2] * s - w2 * cz + d * z], axis=1)


def sample_terms(state, torque_limit, dt, feet=FEET):
    """([13, N] float64 per-step terms, [N] bool ok).  ok False: an input the sample reads is
    non-finite (the terms of that env are meaningless)."""
    S = {k: np.asarray(state[k]).astype(np.float64) for k in STATE_KEYS}
    root, cmd = S["root_states"], S["commands"]
    n = root.shape[0]
    fz = np.stack([S["contact_forces"][:, b, 2] for b in feet], axis=1)
    fv = np.stack([S["rigid_state"][:, b, 7:9] for b in feet], axis=1)          # [N, 2, 2]
    read = np.concatenate([root[:, 3:13], cmd[:, 0:3], S["torques"], S["dof_vel"], S["actions"], S["last_actions"],
                           fz, fv.reshape(n, 4)], axis=1)
    ok = np.isfinite(read).all(axis=1)
    with np.errstate(all="ignore"):
        q = root[:, 3:7]
        qn = 1.0 / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        q = q * qn[:, None]
        vw, ww = root[:, 7:10], root[:, 10:13]
        vb, wb = rotate_inverse(q, vw), rotate_inverse(q, ww)
        gb = rotate_inverse(q, np.tile(np.array([0.0, 0.0, -1.0]), (n, 1)))
        tau, qd, a, ap = S["torques"], S["dof_vel"], S["actions"], S["last_actions"]
        lim = np.asarray(torque_limit, np.float32).astype(np.float64)
        work = np.zeros(n)
        tq2 = np.zeros(n)
        ar2 = np.zeros(n)
        peak = np.zeros(n)
        for j in range(12):
            work = work + np.maximum(tau[:, j] * qd[:, j], 0.0)
            tq2 = tq2 + tau[:, j] * tau[:, j]
            da = a[:, j] - ap[:, j]
            ar2 = ar2 + da * da
            peak = np.maximum(peak, np.abs(tau[:, j]) / lim[j])
        touch = fz > CONTACT_Z
        slip = np.zeros(n)
        for f in range(2):
            slip = slip + np.where(touch[:, f], np.sqrt(fv[:, f, 0] * fv[:, f, 0] + fv[:, f, 1] * fv[:, f, 1]), 0.0)
        T = np.zeros((13, n))
        T[0] = 1.0
        T[1] = (vb[:, 0] - cmd[:, 0]) ** 2
        T[2] = (vb[:, 1] - cmd[:, 1]) ** 2
        T[3] = (wb[:, 2] - cmd[:, 2]) ** 2
        T[4] = np.sqrt(vw[:, 0] * vw[:, 0] + vw[:, 1] * vw[:, 1]) * dt
        T[5] = work * dt
        T[6] = tq2 * dt
        T[7] = gb[:, 0] * gb[:, 0] + gb[:, 1] * gb[:, 1]
        T[8] = slip * dt
        T[9] = ar2
        T[10] = (touch.sum(axis=1) == 2).astype(np.float64)
        T[11] = (touch.sum(axis=1) == 0).astype(np.float64)
        T[12] = peak
    return T, ok


def sample(state, torque_limit, dt, run, counts, feet=FEET):
    """One hg_metrics_sample on copies of run [13, N] / counts [4, N]: returns (run, counts)."""
    run, counts = np.array(run, np.float64), np.array(counts, np.int64)
    T, ok = sample_terms(state, torque_limit, dt, feet)
    run[:12, ok] += T[:12, ok]
    run[12, ok] = np.maximum(run[12, ok], T[12, ok])
    counts[3, ~ok] += 1
    return run, counts


def fold(run, done, counts, mode, reset=None, time_out=None, mask=None):
    """One hg_metrics_fold on copies: returns (run, done, counts)."""
    run, done, counts = np.array(run, np.float64), np.array(done, np.float64), np.array(counts, np.int64)
    n = run.shape[1]
    if mode == 1:
        sel = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
        run[:, sel] = 0.0
        return run, done, counts
    assert mode == 0
    end = np.asarray(reset).astype(bool) & (run[0] > 0)
    to = np.asarray(time_out).astype(bool)
    done[:12, end] += run[:12, end]
    done[12, end] = np.maximum(done[12, end], run[12, end])
    counts[0, end] += 1
    counts[1, end & ~to] += 1
    counts[2, end & to] += 1
    run[:, end] = 0.0
    return run, done, counts


def max_deviation(got, want):
    """Largest |got - want| / (ATOL + RTOL |want|): <= 1 passes the issue's bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (ATOL + RTOL * np.abs(want)))) if got.size else 0.0
