"""Time the stride detector's launches with HIP events through env.kernel_timer: two envs of 4096 in
one process, one with metrics.gait alone and one with metrics.strides as well, stepped alternately
with the same random actions.  The "k_metrics_sample" / "k_metrics_fold" brackets of the first hold
the metrics kernel alone, those of the second the metrics kernel followed by the stride kernel, so
the stride kernels' cost is the difference of the two (the event pair's own floor, "empty", cancels).
Prints one JSON line and, with --out, writes it to that file.

    python scripts/stride_timing.py [--envs 4096] [--steps 300] [--out profiles/strides/timing.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "humanoid-gym-with-comments_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from metrics_timing import Timer  # noqa: E402


def make_env(n, strides):
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.utils.helpers import SimParams
    torch.manual_seed(5)
    np.random.seed(5)
    cfg = XBotLCfg()
    cfg.env.num_envs = n
    cfg.seed = 5
    cfg.metrics.gait = True
    cfg.metrics.strides = strides
    env = XBotLFreeEnv(cfg, SimParams(), "hg_sim", "cuda:0", True)
    env.kernel_timer = Timer()
    return env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    envs = {"gait": make_env(args.envs, False), "gait_strides": make_env(args.envs, True)}
    acts = [torch.randn(args.envs, 12, device="cuda:0") * 0.3 for _ in range(8)]
    for k in range(args.warmup + args.steps):
        if k == args.warmup:
            torch.cuda.synchronize()
            for env in envs.values():
                env.kernel_timer.enabled = True
        for env in envs.values():
            env.step(acts[k % 8])
            env.kernel_timer.start("empty")
            env.kernel_timer.stop("empty")
    torch.cuda.synchronize()
    result = {"envs": args.envs, "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    for key, env in envs.items():
        result[key] = {name: env.kernel_timer.stats(name)
                       for name in ("k_step", "k_metrics_sample", "k_post", "k_metrics_fold", "empty")}
    med = lambda key, name: result[key][name]["median_us"]  # noqa: E731
    floor = med("gait", "empty")
    metrics = med("gait", "k_metrics_sample") + med("gait", "k_metrics_fold") - 2 * floor
    both = med("gait_strides", "k_metrics_sample") + med("gait_strides", "k_metrics_fold") - 2 * med("gait_strides", "empty")
    result["k_metrics_sample_plus_fold_us"] = metrics
    result["k_stride_sample_plus_fold_us"] = both - metrics
    result["k_stride_sample_us"] = med("gait_strides", "k_metrics_sample") - med("gait", "k_metrics_sample")
    result["k_stride_fold_us"] = med("gait_strides", "k_metrics_fold") - med("gait", "k_metrics_fold")
    result["stride_over_metrics"] = (both - metrics) / metrics
    result["stride_report"] = envs["gait_strides"].stride_report()["both"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
