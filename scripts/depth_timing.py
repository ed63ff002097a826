"""Time hg_render_depth with HIP events: 4096 envs on the heightfield, at the poses a seeded
rollout reaches after 24 steps, at 106 x 60 and 16 x 12 pixels, for both pixel-to-lane mappings
(8 x 8 tile per wave, the default; 64 row-major pixels per wave, HG_DEPTH_MAP=rows).  The two
mappings alternate launch by launch, so they see the same machine state; also checks that they
render the same image.  Prints one JSON line and, with --out, writes it to that file.

    python scripts/depth_timing.py [--envs 4096] [--reps 30] [--out profiles/depth/render_times.json]

--robot times hg_render_depth_robot (depth.draw_robot: the robot's legs in view) against
hg_render_depth instead, launch by launch alternating, at 106 x 60: once with the pitches drawn from
depth.angle and once with every pitch at --robot-pitch degrees.  It also reports the share of pixels
the legs change, the share of 8 x 8 tiles holding such a pixel, and the share of tiles that tested
at least one shape: the tiles met by a shape's pixel rectangle, the rectangles recomputed on the host
(a float64 restatement of hd_pixel_rect, csrc/hg_depth_robot.h) from hg_view_shapes' rows.

    python scripts/depth_timing.py --robot [--robot-pitch 60] [--out profiles/depth/robot_times.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "humanoid-gym-with-comments_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--robot", action="store_true")
    ap.add_argument("--robot-pitch", type=float, default=60.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.utils.helpers import SimParams

    torch.manual_seed(5)
    np.random.seed(5)
    cfg = XBotLCfg()
    cfg.env.num_envs = args.envs
    cfg.seed = 5
    cfg.terrain.mesh_type = "heightfield"
    cfg.depth.use_camera = True
    env = XBotLFreeEnv(cfg, SimParams(), "hg_sim", "cuda:0", True)
    for _ in range(args.steps):
        env.step(torch.randn(args.envs, 12, device="cuda:0") * 0.3)
    torch.cuda.synchronize()
    lib = N.lib()
    result = {"envs": args.envs, "steps": args.steps, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    if args.robot:
        robot_timing(args, env, cfg, lib, N, result)
    for w, h in (() if args.robot else ((106, 60), (16, 12))):
        cfg.depth.original = (w, h)
        cam = N.depth_cam(cfg.depth)
        outs = {m: torch.empty(args.envs, h, w, device="cuda:0") for m in ("tile", "rows")}
        times = {m: [] for m in outs}

        def launch(m):
            N.check(lib.hg_render_depth(env.sim, ctypes.byref(cam), N.ptr(env.depth_cam_pitch), N.ptr(outs[m]),
                                        ctypes.c_int64(h * w), ctypes.c_uint64(0), N.stream_ptr(env.device)), env.sim)
        for m in outs:  # warm-up: code object load
            os.environ["HG_DEPTH_MAP"] = m
            launch(m)
            launch(m)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for m in outs:
                os.environ["HG_DEPTH_MAP"] = m
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(m)
                b.record()
                b.synchronize()
                times[m].append(a.elapsed_time(b))
        os.environ.pop("HG_DEPTH_MAP", None)
        same = bool(torch.equal(outs["tile"], outs["rows"]))
        hit = float((outs["tile"] < 0.5).float().mean())
        for m in outs:
            t = np.asarray(times[m])
            result[f"{w}x{h}_{m}_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}
        result[f"{w}x{h}_mappings_equal"] = same
        result[f"{w}x{h}_terrain_pixel_share"] = hit
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


def tested_tile_share(env, cfg, w, h):
    """Share of (env, 8 x 8 tile) pairs whose tile meets the pixel rectangle of at least one drawn
    shape, and the mean number of shapes tested per tile: hd_pixel_rect restated in float64."""
    rows = env.view_shapes().double().cpu().numpy()                    # [N, ns, 16] world rows
    body0 = {6, 7, 10}                                                 # XBot-L: hands and base box sit on body 0
    rows = rows[:, [k for k in range(rows.shape[1]) if k not in body0]]
    root = env.root_states.double().cpu().numpy()
    q = root[:, 3:7] / np.linalg.norm(root[:, 3:7], axis=1, keepdims=True)
    x, y, z, qw = q.T
    Rb = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * qw), 2 * (x * z + y * qw)], -1),
                   np.stack([2 * (x * y + z * qw), 1 - 2 * (x * x + z * z), 2 * (y * z - x * qw)], -1),
                   np.stack([2 * (x * z - y * qw), 2 * (y * z + x * qw), 1 - 2 * (x * x + y * y)], -1)], 1)
    p = env.depth_cam_pitch.double().cpu().numpy()
    cp, sp, zero, one = np.cos(p), np.sin(p), np.zeros_like(p), np.ones_like(p)
    Ry = np.stack([np.stack([cp, zero, sp], -1), np.stack([zero, one, zero], -1), np.stack([-sp, zero, cp], -1)], 1)
    R = Rb @ Ry                                                        # columns: fwd, left, up
    o = root[:, :3] + np.einsum("nij,j->ni", Rb, np.asarray(cfg.depth.position, np.float64))
    cap = rows[..., 0] == 0
    a, b = rows[..., 1:4], rows[..., 4:7]
    ctr = np.where(cap[..., None], (a + b) / 2, a) - o[:, None]
    rho = np.where(cap, np.linalg.norm(b - a, axis=-1) / 2 + rows[..., 7], np.linalg.norm(b, axis=-1)) * 1.0001 + 1e-5
    cam = np.einsum("nji,nsj->nsi", R, ctr)                            # camera-frame x, y, z
    xc, yc, zc = cam[..., 0], cam[..., 1], cam[..., 2]
    fx = (w / 2) / np.tan(np.deg2rad(float(cfg.depth.horizontal_fov)) / 2)
    xl, xh = np.maximum(xc - rho, 1e-30), xc + rho

    def bounds(v):
        vl, vh = v - rho, v + rho
        return np.where(vl < 0, vl / xl, vl / xh), np.where(vh > 0, vh / xl, vh / xh)
    ylo, yhi = bounds(yc)
    zlo, zhi = bounds(zc)
    c0 = np.floor(np.clip(w / 2 - yhi * fx - 0.5, -2, w + 2)) - 1
    c1 = np.ceil(np.clip(w / 2 - ylo * fx - 0.5, -2, w + 2)) + 1
    r0 = np.floor(np.clip(h / 2 - zhi * fx - 0.5, -2, h + 2)) - 1
    r1 = np.ceil(np.clip(h / 2 - zlo * fx - 0.5, -2, h + 2)) + 1
    whole = ~np.isfinite(xc + yc + zc + rho) | ((xc + rho >= 0) & (xc - rho <= 0))
    r0, c0 = np.where(whole, 0, np.maximum(r0, 0)), np.where(whole, 0, np.maximum(c0, 0))
    r1, c1 = np.where(whole, h - 1, np.minimum(r1, h - 1)), np.where(whole, w - 1, np.minimum(c1, w - 1))
    empty = ~whole & ((xc + rho < 0) | (r0 > r1) | (c0 > c1))
    tr = np.arange((h + 7) // 8) * 8
    tc = np.arange((w + 7) // 8) * 8
    rows_hit = ~empty[..., None] & (r1[..., None] >= tr) & (r0[..., None] <= tr + 7)   # [N, ns, tiles_y]
    cols_hit = ~empty[..., None] & (c1[..., None] >= tc) & (c0[..., None] <= tc + 7)   # [N, ns, tiles_x]
    per_tile = (rows_hit[..., :, None] & cols_hit[..., None, :]).sum(1)                # shapes tested per tile
    return float((per_tile > 0).mean()), float(per_tile.mean())


def robot_timing(args, env, cfg, lib, N, result):
    w, h = cfg.depth.original
    cam = N.depth_cam(cfg.depth, normalize=False)
    entries = {"terrain": lib.hg_render_depth, "robot": lib.hg_render_depth_robot}
    outs = {m: torch.empty(args.envs, h, w, device="cuda:0") for m in entries}
    drawn = env.depth_cam_pitch.clone()
    for label, pitch in (("default_pitch", drawn), (f"pitch_{args.robot_pitch:g}", torch.full_like(drawn, float(np.deg2rad(args.robot_pitch))))):
        env.depth_cam_pitch.copy_(pitch)
        times = {m: [] for m in entries}

        def launch(m):
            N.check(entries[m](env.sim, ctypes.byref(cam), N.ptr(env.depth_cam_pitch), N.ptr(outs[m]),
                               ctypes.c_int64(h * w), ctypes.c_uint64(0), N.stream_ptr(env.device)), env.sim)
        for m in entries:  # warm-up: code object load
            launch(m)
            launch(m)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for m in entries:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch(m)
                b.record()
                b.synchronize()
                times[m].append(a.elapsed_time(b))
        for m in entries:
            t = np.asarray(times[m])
            result[f"{label}_{m}_ms"] = {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}
        changed = outs["robot"] != outs["terrain"]
        assert bool((outs["robot"] <= outs["terrain"]).all())   # a leg only ever brings a pixel nearer
        pad = torch.zeros(args.envs, (h + 7) // 8 * 8, (w + 7) // 8 * 8, dtype=torch.bool, device="cuda:0")
        pad[:, :h, :w] = changed
        tiles = pad.view(args.envs, pad.shape[1] // 8, 8, pad.shape[2] // 8, 8).any(4).any(2)
        result[f"{label}_robot_pixel_share"] = float(changed.float().mean())
        result[f"{label}_robot_tile_share"] = float(tiles.float().mean())
        result[f"{label}_envs_with_robot_pixels"] = float(changed.flatten(1).any(1).float().mean())
        share, mean = tested_tile_share(env, cfg, w, h)
        result[f"{label}_tiles_testing_a_shape"] = share
        result[f"{label}_shapes_tested_per_tile"] = mean
    env.depth_cam_pitch.copy_(drawn)


if __name__ == "__main__":
    main()
