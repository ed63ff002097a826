"""Evaluate a policy by its gait, not by its reward: run it on the training env (env.step, the env's
own observation stack, noise, pushes and terrain) with gait metrics on (metrics.gait: sampled and
folded on the device every step) and print / write the report of env.gait_report — command-tracking
RMS errors, distance per episode, cost of transport, foot slip per metre, tilt, support fractions,
peak torque ratio, episodes and the fall rate — overall and per terrain type.

    python -m humanoid.scripts.evaluate --load_model policy_1.pt [--envs 256] [--duration 20]
        [--command VX VY WZ] [--terrain plane|heightfield|trimesh] [--seed 5] [--out DIR] [--strides]

``--load_model`` is read as scripts/sim2sim.py reads it (TorchScript export, ONNX actor or weights
npz).  ``--command`` fixes every env's command for the whole run (no resampling, no heading
command); without it the env samples commands as in training.  Episodes still running when the
duration ends are not part of the report (it covers completed episodes), so the duration should
be longer than env.episode_length_s unless falls are the point.  BUILD-DEFINED: the reference has
no such script.

``--strides`` turns metrics.strides on as well and adds a ``"strides"`` section to the report
(env.stride_report: swing time, foot clearance against rewards.target_feet_height, step length and
width, stride time against rewards.cycle_time, cadence, asymmetry; rows left / right / both, overall
and per terrain type).  Without the flag the output is what it was.
"""
import argparse
import json
import os

import numpy as np
import torch

from humanoid.scripts.sim2sim import load_policy

ROW_ORDER = ["episodes", "falls", "time_outs", "fall_rate", "steps", "skipped", "rms_err_vx", "rms_err_vy", "rms_err_wz",
             "distance_per_episode", "cost_of_transport", "slip_per_metre", "tilt_rms", "double_support_fraction",
             "flight_fraction", "peak_torque_ratio", "mean_torque2", "action_rate_rms"]


STRIDE_ROW_ORDER = ["strides", "strides_per_episode", "mean_swing_time", "mean_clearance", "clearance_vs_target",
                    "mean_step_length", "mean_step_width", "mean_touchdown_force", "mean_stride_length",
                    "mean_stride_time", "stride_time_vs_cycle", "cadence", "swing_fraction", "short_swing_fraction",
                    "swing_time_asymmetry", "step_length_asymmetry"]


def make_cfg(num_envs, duration, command=None, terrain="plane", seed=5, strides=False):
    """XBotLCfg of the training env with gait metrics on (strides: the stride detector as well); a
    fixed command turns resampling and the heading command off."""
    from humanoid.envs import XBotLCfg
    cfg = XBotLCfg()
    cfg.seed = int(seed)
    cfg.env.num_envs = int(num_envs)
    cfg.terrain.mesh_type = terrain
    if terrain == "plane":
        cfg.terrain.curriculum = False
    cfg.metrics.gait = True
    cfg.metrics.strides = bool(strides)
    if command is not None:
        if len(command) != 3:
            raise ValueError(f"--command takes VX VY WZ, got {list(command)}")
        cfg.commands.heading_command = False
        cfg.commands.resampling_time = float(duration) + cfg.env.episode_length_s + 1.0
    return cfg


def evaluate(policy, num_envs=256, duration=20.0, command=None, terrain="plane", seed=5, device="cuda:0", env=None,
             strides=False):
    """Run `policy` (a callable [N, num_obs] -> [N, 12]) for `duration` simulated seconds; returns
    (report, env): env.gait_report(by_terrain_type=True) plus the run's settings and, with strides,
    a "strides" section, env.stride_report(by_terrain_type=True)."""
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.utils.helpers import SimParams
    if env is None:
        torch.manual_seed(seed)
        np.random.seed(seed)
        env = XBotLFreeEnv(make_cfg(num_envs, duration, command, terrain, seed, strides), SimParams(), "hg_sim", device, True)
    if not hasattr(env, "gait_report"):
        raise ValueError("evaluate needs an env with metrics.gait on")
    if strides and not hasattr(env, "stride_report"):
        raise ValueError("evaluate(strides=True) needs an env with metrics.strides on")
    cmd = None if command is None else torch.tensor([float(v) for v in command], dtype=torch.float32, device=env.device)
    steps = int(round(duration / env.dt))
    clip_a = env.cfg.normalization.clip_actions
    env.clear_gait_metrics()
    obs = env.get_observations()
    with torch.no_grad():
        for _ in range(steps):
            if cmd is not None:
                env.commands[:, :3] = cmd
            actions = torch.clamp(policy(obs.detach()).float(), -clip_a, clip_a)
            obs, _, _, _, _ = env.step(actions)
    report = env.gait_report(by_terrain_type=True)
    if strides:
        report["strides"] = env.stride_report(by_terrain_type=True)
    report["settings"] = dict(envs=env.num_envs, duration_s=float(duration), steps=steps, policy_dt=float(env.dt),
                              command=None if command is None else [float(v) for v in command],
                              terrain=env.cfg.terrain.mesh_type, seed=int(seed))
    return report, env


def format_report(report):
    """The report as a text table: one column overall, one per terrain type."""
    cols = [("overall", report["overall"])] + [(f"type {k}", r) for k, r in sorted(report["terrain_types"].items())]
    if len(cols) == 2:
        cols = cols[:1]  # a single terrain type is the overall column again

    def cell(v):
        if v is None:
            return "-"
        return f"{v:d}" if isinstance(v, (int, np.integer)) else f"{v:.4f}"
    names = [k for k in ROW_ORDER if k in report["overall"]] + sorted(set(report["overall"]) - set(ROW_ORDER))
    width = max(len(n) for n in names)
    lines = [" " * width + "".join(f"{title:>14s}" for title, _ in cols)]
    for n in names:
        lines.append(f"{n:<{width}s}" + "".join(f"{cell(r.get(n)):>14s}" for _, r in cols))
    return "\n".join(lines)


def format_stride_report(report):
    """env.stride_report(by_terrain_type=True) as text: the left / right / both table overall, then
    one per terrain type (none when there is a single type)."""
    def cell(v):
        if v is None:
            return "-"
        return f"{v:d}" if isinstance(v, (int, np.integer)) else f"{v:.4f}"

    def table(title, rows):
        cols = ["left", "right", "both"]
        width = max(len(n) for n in STRIDE_ROW_ORDER)
        lines = [f"{title:<{width}s}" + "".join(f"{c:>14s}" for c in cols)]
        for n in STRIDE_ROW_ORDER:
            lines.append(f"{n:<{width}s}" + "".join(f"{cell(rows[c].get(n)) if n in rows[c] else '':>14s}" for c in cols))
        return lines
    lines = table("overall", report["overall"])
    if len(report["terrain_types"]) > 1:
        for k, rows in sorted(report["terrain_types"].items()):
            lines += table(f"type {k}", rows)
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--load_model", required=True,
                    help="TorchScript actor (exported policy_1.pt), ONNX actor (.onnx) or weights (.npz)")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--duration", type=float, default=20.0, help="seconds of simulated time")
    ap.add_argument("--command", type=float, nargs=3, metavar=("VX", "VY", "WZ"), default=None,
                    help="fixed command for every env (default: the env samples commands as in training)")
    ap.add_argument("--terrain", default="plane", choices=["plane", "heightfield", "trimesh"])
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None, help="output directory (default: next to the policy)")
    ap.add_argument("--strides", action="store_true",
                    help="also run the stride detector (metrics.strides) and add a \"strides\" section")
    a = ap.parse_args(argv)
    policy = load_policy(a.load_model)
    report, _ = evaluate(policy, a.envs, a.duration, a.command, a.terrain, a.seed, strides=a.strides)
    out = a.out or os.path.join(os.path.dirname(os.path.abspath(a.load_model)), "evaluate")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "gait_report.json")
    with open(path, "w") as f:
        doc = {**report, "terrain_types": {str(k): v for k, v in report["terrain_types"].items()}}
        if "strides" in report:
            st = report["strides"]
            doc["strides"] = {**st, "terrain_types": {str(k): v for k, v in st["terrain_types"].items()}}
        json.dump(doc, f, indent=1)
    print(format_report(report))
    if "strides" in report:
        print(format_stride_report(report["strides"]))
    print(f"{report['settings']['envs']} envs x {report['settings']['duration_s']:.1f} s -> {path}")
    return report


if __name__ == "__main__":
    main()
