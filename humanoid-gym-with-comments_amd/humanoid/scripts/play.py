"""Evaluation loop (humanoid/scripts/play.py of the reference), headless.

    python -m humanoid.scripts.play --task humanoid_ppo --load_run <run> --resume [--steps 1000]
        [--record DIR [--record_env K] [--record_every M]]

Loads the checkpoint, exports the actor (TorchScript policy_1.pt + base_lin_vel.pt, and ONNX
policy.onnx), runs the policy on a single environment with the reference's play settings and
writes the open-loop action trace (openloop_action.npz) plus per-step state logs (states.npz) and
the mean episode rewards.

``--record DIR`` films the rollout as the reference does with its camera sensor (play.py:84-141):
after every ``--record_every``-th step the follow camera of ``cfg.viewer`` (env.render_view: robot
shapes and terrain ray-cast by hg_render_view) renders env ``--record_env`` and the frame is written
as ``DIR/frame_%05d.png``; when ``cv2`` is importable the frames also go into ``DIR/play.mp4``.  With
``--record`` play keeps the task's own terrain type instead of forcing the plane, so stairs can be
filmed.  There is no interactive viewer.

With ``metrics.gait`` on in the task's config play ends by printing env.gait_report (tracking errors,
cost of transport, slip, fall rate, ...) over the episodes the rollout completed; with
``metrics.strides`` as well, env.stride_report (clearance, step length, stride time, cadence, ...).

Reference defect fixed: play.py:77 sets ``train_cfg.runner.resume = True``, but
``make_alg_runner`` resets it to False before reading it (task_registry.py:137), so without an
explicit ``--resume`` the reference exports and plays the randomly initialised policy.  Here the
resume request travels in ``args``, which make_alg_runner honours: play always loads the
checkpoint (``--load_run`` / ``--checkpoint``, default the newest).
"""
import argparse
import os

import numpy as np
import torch

from humanoid import LEGGED_GYM_ROOT_DIR
from humanoid.envs import *  # noqa: F401,F403
from humanoid.utils import get_args, task_registry
from humanoid.utils.helpers import export_policy_as_jit
from humanoid.utils.onnx_io import export_policy_as_onnx

EXPORT_POLICY = True
FIX_COMMAND = True


def _video_writer(path, size, fps):
    """cv2.VideoWriter for play.mp4, or None when cv2 is not installed (the frames are the record)."""
    try:
        import cv2
    except ImportError:
        return None
    return cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), fps, size)


def play(args, steps=100, record=None, record_env=0, record_every=1):
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.env.num_envs = min(env_cfg.env.num_envs, 1)
    if record is None:
        env_cfg.terrain.mesh_type = "plane"
    env_cfg.terrain.num_rows = 5
    env_cfg.terrain.num_cols = 5
    env_cfg.terrain.curriculum = False
    env_cfg.terrain.max_init_terrain_level = 5
    env_cfg.noise.add_noise = True
    env_cfg.domain_rand.push_robots = False
    env_cfg.domain_rand.randomize_actuators = False
    env_cfg.noise.noise_level = 0.5
    train_cfg.seed = 123145
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    obs = env.get_observations()
    train_cfg.runner.resume = True
    args.resume = True  # see the module docstring (task_registry.py:137 would drop the line above)
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg)
    policy = runner.get_inference_policy(device=env.device)
    root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", train_cfg.runner.experiment_name)
    if EXPORT_POLICY:
        path = os.path.join(root, "exported", "policies")
        export_policy_as_jit(runner.alg.actor_critic, path)
        export_policy_as_onnx(runner.alg.actor_critic, path)
        print("Exported policy (TorchScript + ONNX) to:", path)
    actions_log, states = [], {k: [] for k in ("dof_pos", "dof_vel", "dof_torque", "command_x", "base_vel_x",
                                               "base_vel_yaw", "contact_forces_z")}
    rew_sums, n_eps = {}, 0
    video, frames = None, 0
    if record is not None:
        if not 0 <= record_env < env.num_envs:
            raise ValueError(f"--record_env must be in [0, {env.num_envs}), got {record_env}")
        if record_every < 1:
            raise ValueError(f"--record_every must be >= 1, got {record_every}")
        from humanoid.utils.png import write_png
        os.makedirs(record, exist_ok=True)
        cam = env.default_view_cam(follow=True, n=1)
        frame = torch.empty(1, cam.height, cam.width, 3, dtype=torch.uint8, device=env.device)
        video = _video_writer(os.path.join(record, "play.mp4"), (cam.width, cam.height), 1.0 / (env.dt * record_every))
    for it in range(steps):
        with torch.no_grad():
            actions = policy(obs.detach())
        actions_log.append(actions[0].cpu().numpy())
        if FIX_COMMAND:
            env.commands[:, 0] = 0.5
            env.commands[:, 1:4] = 0.0
        obs, _, _, _, infos = env.step(actions.detach())
        states["dof_pos"].append(env.dof_pos[0].cpu().numpy())
        states["dof_vel"].append(env.dof_vel[0].cpu().numpy())
        states["dof_torque"].append(env.torques[0].cpu().numpy())
        states["command_x"].append(float(env.commands[0, 0]))
        states["base_vel_x"].append(float(env.base_lin_vel[0, 0]))
        states["base_vel_yaw"].append(float(env.base_ang_vel[0, 2]))
        states["contact_forces_z"].append(env.contact_forces[0, env.feet_indices, 2].cpu().numpy())
        if record is not None and (it + 1) % record_every == 0:
            env.render_view(env_ids=[record_env], cam=cam, rgb=frame)
            img = frame[0].cpu().numpy()
            write_png(os.path.join(record, "frame_%05d.png" % frames), img)
            if video is not None:
                video.write(img[:, :, ::-1].copy())  # BGR
            frames += 1
        k = int(env.reset_buf.sum().item())
        if k > 0:
            n_eps += k
            for name, v in infos["episode"].items():
                rew_sums[name] = rew_sums.get(name, 0.0) + float(v) * k
    out = os.path.join(root, "openloop_action")
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "openloop_action.npz"), action=np.array(actions_log))
    np.savez(os.path.join(out, "states.npz"), **{k: np.array(v) for k, v in states.items()})
    if video is not None:
        video.release()
    if record is not None:
        print(f"Recorded {frames} frames to:", record)
    if n_eps:
        print(f"Average rewards per second over {n_eps} episodes:")
        for name, v in rew_sums.items():
            print(f" - {name}: {v / n_eps:.4f}")
    if hasattr(env, "gait_report"):  # metrics.gait: the completed episodes' gait figures
        from humanoid.scripts.evaluate import format_report
        print("Gait metrics over the completed episodes:")
        print(format_report(env.gait_report(by_terrain_type=True)))
    if hasattr(env, "stride_report"):  # metrics.strides: the completed episodes' stride figures
        from humanoid.scripts.evaluate import format_stride_report
        print("Stride statistics over the completed episodes:")
        print(format_stride_report(env.stride_report(by_terrain_type=True)))
    return np.array(actions_log)


def record_parser():
    """play's own flags; what it does not know goes on to get_args."""
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--record", metavar="DIR", default=None, help="write follow-camera frames (PNG) into DIR")
    ap.add_argument("--record_env", type=int, default=0, help="the env to film")
    ap.add_argument("--record_every", type=int, default=1, help="film every M-th step")
    return ap


if __name__ == "__main__":
    extra, rest = record_parser().parse_known_args()
    play(get_args(rest), steps=extra.steps, record=extra.record, record_env=extra.record_env,
         record_every=extra.record_every)
