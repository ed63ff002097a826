"""numpy references of the rollout-side kernels (csrc/hg_rollout.hip).  TEST INFRASTRUCTURE ONLY:
nothing here imports the package.

  act_normals / act_normals64  the action noise of hg_rollout_act: Philox keyed by (seed,
                               env + row_offset, counter, block j >> 2, purpose 9), Box-Muller
  log_prob64                   the Normal log-density summed over actions, and its magnitude sum
  bootstrap64                  the time-out bootstrap of hg_rollout_env
  stack_replay                 the observation deque of the reference env, stepped literally (what
                               hg_gather_stacked rebuilds from frame-only storage)
"""
import numpy as np

import rng_ref as R

ACTION_SAMPLE = 9  # RNG_ACTION_SAMPLE of csrc/hg_rollout.hip

TWO_PI_F32 = np.float32(6.283185307179586)
LOG_SQRT_2PI = 0.91893853320467274178


def _draws(seed, row_offset, counter, n, A):
    """The uint32 Philox outputs of every 4-action block: list over blocks of 4 arrays [n]."""
    env = np.arange(n, dtype=np.uint64) + np.uint64(row_offset)
    return [R.rng4(seed, env, counter, b, ACTION_SAMPLE) for b in range((A + 3) // 4)]


def act_normals(seed, row_offset, counter, n, A):
    """float32 z [n, A] as normals4() of hg_common.h computes them (numpy float32 libm)."""
    return np.concatenate([R.normals4(r) for r in _draws(seed, row_offset, counter, n, A)], 1)[:, :A]


def act_normals64(seed, row_offset, counter, n, A):
    """(z, radius), both float64 [n, A], from the same uint32 draws: u and the angle are formed in
    float32 exactly as u01_open0, u01 and two_pi * u do; log, sqrt, sin and cos are float64."""
    zs, rs = [], []
    for r in _draws(seed, row_offset, counter, n, A):
        r0 = np.sqrt(-2.0 * np.log(R.u01_open0(r[0]).astype(np.float64)))
        r1 = np.sqrt(-2.0 * np.log(R.u01_open0(r[2]).astype(np.float64)))
        a0 = (TWO_PI_F32 * R.u01(r[1])).astype(np.float32).astype(np.float64)
        a1 = (TWO_PI_F32 * R.u01(r[3])).astype(np.float32).astype(np.float64)
        zs.append(np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], 1))
        rs.append(np.stack([r0, r0, r1, r1], 1))
    return np.concatenate(zs, 1)[:, :A], np.concatenate(rs, 1)[:, :A]


def log_prob64(a, mu, sigma):
    """(log p(a), S): sum_j [-(a_j - mu_j)^2 / (2 sigma_j^2) - ln sigma_j - ln sqrt(2 pi)] in float64
    and the magnitude sum S = sum_j (|d_j^2 / (2 sigma_j^2)| + |ln sigma_j| + ln sqrt(2 pi)), per row."""
    a, mu, sigma = (np.asarray(x, dtype=np.float64) for x in (a, mu, sigma))
    q = (a - mu) ** 2 / (2.0 * sigma ** 2)
    ls = np.log(sigma)
    return (-q - ls - LOG_SQRT_2PI).sum(-1), (np.abs(q) + np.abs(ls) + LOG_SQRT_2PI).sum(-1)


def bootstrap64(r, v, time_out, gamma):
    """rewards + gamma * V * time_out (ppo.py:132-133) in float64; gamma is the float32 the ABI takes."""
    g = float(np.float32(gamma))
    return np.asarray(r, np.float64) + g * np.asarray(v, np.float64) * np.asarray(time_out, np.float64)


def stack_replay(init, frames, dones, F, W):
    """The reference's observation deque, stepped literally.  init [N, F W] is the stack at step 0
    (its newest frame is frames[0]), frames [T, N, W] the newest frame of every step, dones [T, N]
    the resets of every step.  Returns stack [T, N, F W]:
      stack[0] = init;  stack[t + 1] = concat(0 if dones[t] else stack[t][:, W:], frames[t + 1])."""
    init, frames, dones = np.asarray(init), np.asarray(frames), np.asarray(dones)
    T, N = frames.shape[:2]
    assert init.shape == (N, F * W) and frames.shape == (T, N, W) and dones.shape == (T, N)
    out = np.empty((T, N, F * W), dtype=frames.dtype)
    out[0] = init
    for t in range(T - 1):
        hist = np.where(dones[t].astype(bool)[:, None], np.zeros_like(out[t][:, W:]), out[t][:, W:])
        out[t + 1] = np.concatenate([hist, frames[t + 1]], 1)
    return out
