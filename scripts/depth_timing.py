"""Time hg_render_depth with HIP events: 4096 envs on the heightfield, at the poses a seeded
rollout reaches after 24 steps, at 106 x 60 and 16 x 12 pixels, for both pixel-to-lane mappings
(8 x 8 tile per wave, the default; 64 row-major pixels per wave, HG_DEPTH_MAP=rows).  The two
mappings alternate launch by launch, so they see the same machine state; also checks that they
render the same image.  Prints one JSON line and, with --out, writes it to that file.

    python scripts/depth_timing.py [--envs 4096] [--reps 30] [--out profiles/depth/render_times.json]
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
    for w, h in ((106, 60), (16, 12)):
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


if __name__ == "__main__":
    main()
