"""Generate tests/golden/cmd_curriculum.npz from the REFERENCE implementation's command curriculum.

Runs only where the reference tree is available (as tests/golden/gen_goldens.py, whose isaacgym
stubs and bare-env helpers it imports); the test suite reads the .npz only.

The reference's ``reset_idx`` (humanoid_env.py:1109-1163) is called on a bare XBotLFreeEnv with
planted ``tracking_lin_vel`` episode sums.  On steps where ``common_step_counter %
max_episode_length == 0`` it runs ``update_command_curriculum`` (:1097-1106) BEFORE it redraws the
resetting envs' commands (:1120-1129) and then publishes ``extras["episode"]["max_command_x"]``
(:1148-1149).  Recorded per case: the inputs (sums of every env, the resetting ids, the counter,
the range going in, max_curriculum), the range coming out, max_command_x, and the raw command
draws with the commands they produced (which shows the draw used the widened range).

Cases (threshold on the mean sum at the defaults: 0.8 x 1.2 x 0.01 x 2400 = 23.04):
  above      mean 2 % above the threshold: the range widens
  below      mean 2 % below: unchanged
  chain0..2  three consecutive firings from [-0.3, 0.6] with max_curriculum 1.0
             (-> [-0.8, 1.0] -> [-1, 1] -> unchanged)
  offstep    high sums, counter 2401 (no multiple of max_episode_length): unchanged
  initial    the counter-0 reset of every env with zero sums: unchanged
In every case the non-resetting envs carry sums that would flip the decision if averaged in.

Usage:  python tests/golden/gen_cmd_curriculum.py
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_goldens as G  # noqa: E402

N = 24
THRESH = 0.8 * 1.2 * 0.01 * 2400  # 23.04


def _case(he, out, tag, seed, counter, ids, mean, rng, max_curriculum, other):
    """One reset_idx call; mean: the mean tracking_lin_vel sum planted on `ids`, `other`: the sum
    planted on every other env."""
    E, g = G._pipeline_env(he, N, seed, False)
    c = E.cfg
    c.commands.curriculum = True
    c.commands.max_curriculum = max_curriculum
    E.command_ranges["lin_vel_x"] = list(rng)
    E.common_step_counter = counter
    ids = np.asarray(ids, np.int64)
    sums = np.full(N, other, np.float32)
    # spread around the mean (sum of the offsets is zero) so a kernel reading one env's sum differs
    off = (np.arange(len(ids)) - (len(ids) - 1) / 2.0) * 0.25
    sums[ids] = (mean + off).astype(np.float32)
    E.episode_sums["tracking_lin_vel"][:] = torch.from_numpy(sums)
    with G.DrawRecorder(he, seed + 100) as rec:
        E.reset_idx(torch.from_numpy(ids))
    p = f"{tag}/"
    out[p + "sums"] = sums
    out[p + "ids"] = ids
    out[p + "counter"] = np.int64(counter)
    out[p + "range_in"] = np.asarray(rng, np.float64)
    out[p + "max_curriculum"] = np.float64(max_curriculum)
    out[p + "max_episode_length"] = np.float64(E.max_episode_length)
    out[p + "reward_scale"] = np.float64(E.reward_scales["tracking_lin_vel"])  # x dt already
    out[p + "range_out"] = np.asarray(E.command_ranges["lin_vel_x"], np.float64)
    out[p + "max_command_x"] = np.float64(E.extras["episode"]["max_command_x"])
    out[p + "range_y"] = np.asarray(E.command_ranges["lin_vel_y"], np.float64)
    draws = rec.rec["reset:cmd"]  # x, y, heading uniforms, each [len(ids), 1]
    out[p + "cmd_u"] = np.stack([d[:, 0] for d in draws[:3]], 1)
    out[p + "commands"] = E.commands[torch.from_numpy(ids)].numpy().copy()
    return list(E.command_ranges["lin_vel_x"])


def main():
    torch.set_num_threads(1)
    G.install_stubs()
    from humanoid.envs.custom import humanoid_env as he
    out = {}
    some = [0, 1, 2, 5, 17, 23]
    _case(he, out, "above", 41, 2400, some, THRESH * 1.02, [-0.3, 0.6], 2.0, other=0.0)
    _case(he, out, "below", 42, 2400, some, THRESH * 0.98, [-0.3, 0.6], 2.0, other=40.0)
    rng = [-0.3, 0.6]
    for k in range(3):
        rng = _case(he, out, f"chain{k}", 43 + k, 2400 * (k + 1), some, THRESH * 1.05, rng, 1.0, other=0.0)
    _case(he, out, "offstep", 46, 2401, some, THRESH * 1.5, [-0.3, 0.6], 1.0, other=40.0)
    _case(he, out, "initial", 47, 0, list(range(N)), 0.0, [-0.3, 0.6], 1.0, other=0.0)
    out["cases"] = np.asarray(["above", "below", "chain0", "chain1", "chain2", "offstep", "initial"])
    np.savez_compressed(os.path.join(HERE, "cmd_curriculum.npz"), **out)
    for t in out["cases"]:
        print(t, out[t + "/range_in"], "->", out[t + "/range_out"], "max_command_x", out[t + "/max_command_x"])


if __name__ == "__main__":
    main()
