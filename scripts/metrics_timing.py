"""Time the gait-metrics launches with HIP events through env.kernel_timer: 4096 envs with
metrics.gait on, random actions, every step's k_step / k_metrics_sample / k_post / k_metrics_fold
bracketed by an event pair (an event pair around an empty stream section costs a few microseconds
itself: "empty" measures that floor in the same run).  Prints one JSON line and, with --out, writes
it to that file.

    python scripts/metrics_timing.py [--envs 4096] [--steps 300] [--out profiles/metrics/timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "humanoid-gym-with-comments_amd"))


class Timer:
    """env.kernel_timer: start(name) / stop(name) record an event pair on the current stream."""

    def __init__(self):
        self.pairs = {}
        self.enabled = False

    def start(self, name):
        if self.enabled:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.pairs.setdefault(name, []).append([e, None])

    def stop(self, name):
        if self.enabled:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.pairs[name][-1][1] = e

    def stats(self, name):
        t = np.asarray([a.elapsed_time(b) * 1e3 for a, b in self.pairs[name]])
        return {"median_us": float(np.median(t)), "mean_us": float(t.mean()), "min_us": float(t.min()), "calls": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.utils.helpers import SimParams

    torch.manual_seed(5)
    np.random.seed(5)
    cfg = XBotLCfg()
    cfg.env.num_envs = args.envs
    cfg.seed = 5
    cfg.metrics.gait = True
    env = XBotLFreeEnv(cfg, SimParams(), "hg_sim", "cuda:0", True)
    timer = Timer()
    env.kernel_timer = timer
    acts = [torch.randn(args.envs, 12, device="cuda:0") * 0.3 for _ in range(8)]
    for k in range(args.warmup):
        env.step(acts[k % 8])
    torch.cuda.synchronize()
    timer.enabled = True
    for k in range(args.steps):
        env.step(acts[k % 8])
        timer.start("empty")
        timer.stop("empty")
    torch.cuda.synchronize()
    result = {"envs": args.envs, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for name in ("k_step", "k_metrics_sample", "k_post", "k_metrics_fold", "empty"):
        result[name] = timer.stats(name)
    rep = env.gait_report()
    result["report"] = rep
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
