"""Learn time of PPO.update with and without the mirror-symmetry loss at the bench's size (4096 envs
x 24 steps, 4 minibatches x 2 epochs, fp32, the production networks), by HIP events around
update() after the capture:

  off     sym_loss=False                                 (the one-graph update)
  fused   sym_loss=True, the fused route                  (mirror gather, second actor pass and the
                                                          symmetry kernels inside the one graph)
  eager   sym_loss=True, use_fused_loss=False             (the op-by-op expression with the dense
                                                          705 x 705 mirror product, eager: what
                                                          sym_loss=True ran before the fused route)

The three alternate in one process, ROUNDS rounds of UPDATES updates each after a warm-up; prints
one JSON line with the per-update mean of each round and over all rounds.  Run the command twice to
see the spread between processes.

Usage:  python scripts/sym_loss_timing.py [--rounds 5] [--updates 10] [--modes off,fused,eager] [--out FILE]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "humanoid-gym-with-comments_amd"))
import torch  # noqa: E402

from humanoid.algo.ppo import ActorCritic, PPO  # noqa: E402
from humanoid.utils.blas_tuning import use_tuned_gemms  # noqa: E402
from humanoid.utils.symmetry import xbotl_mirror  # noqa: E402

N_ENVS, T = 4096, 24
DIMS = dict(num_actor_obs=705, num_critic_obs=219, num_actions=12, actor_hidden_dims=[512, 256, 128],
            critic_hidden_dims=[768, 256, 128], base_lin_vel_hidden_dims=[128, 128], init_noise_std=1.0)
PPO_KW = dict(num_learning_epochs=2, num_mini_batches=4, clip_param=0.2, gamma=0.994, lam=0.9, value_loss_coef=1.0,
              entropy_coef=0.001, learning_rate=1e-5, max_grad_norm=1.0, use_clipped_value_loss=True,
              schedule="adaptive", desired_kl=0.01)


def make(mode, data):
    torch.manual_seed(0)
    ac = ActorCritic(**DIMS)
    kw = dict(PPO_KW)
    if mode != "off":
        obs_perm, act_perm = xbotl_mirror()
        kw.update(sym_loss=True, sym_coef=1.0, obs_permutation=obs_perm, act_permutation=act_perm, frame_stack=15)
    ppo = PPO(ac, device="cuda:0", **kw)
    if mode == "eager":
        ppo.use_fused_loss = False
    ppo.init_storage(N_ENVS, T, [705], [219], [12])

    def load():
        st = ppo.storage
        for k, v in data.items():
            getattr(st, k).copy_(v)
        st.step = T
    return ppo, load


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--modes", default="off,fused,eager", help="subset to run (a kernel trace of one mode)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    use_tuned_gemms()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    sigma = torch.ones(T, N_ENVS, 12, device=dev)
    mu = 0.02 * r(T, N_ENVS, 12)
    actions = mu + sigma * r(T, N_ENVS, 12)
    logp = (-0.5 * (actions - mu) ** 2 - 0.9189385332046727).sum(-1, keepdim=True)
    values = 0.5 * r(T, N_ENVS, 1)
    data = dict(observations=r(T, N_ENVS, 705), privileged_observations=r(T, N_ENVS, 219), actions=actions,
                values=values, actions_log_prob=logp, mu=mu, sigma=sigma, returns=values + 0.5 * r(T, N_ENVS, 1),
                advantages=r(T, N_ENVS, 1))
    modes = tuple(args.modes.split(","))
    runs = {m: make(m, data) for m in modes}
    for m in modes:  # the eager first update, the capture, one replay
        ppo, load = runs[m]
        for _ in range(3):
            load()
            ppo.update(sync=False)
    torch.cuda.synchronize()
    forms = {m: runs[m][0].update_graph for m in modes}
    assert all(forms[m] == ("eager" if m == "eager" else "one") for m in modes), forms
    per_round = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            ppo, load = runs[m]
            ms = 0.0
            for _ in range(args.updates):
                load()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ppo.update(sync=False)
                e1.record()
                e1.synchronize()
                ms += e0.elapsed_time(e1)
            per_round[m].append(ms / args.updates)
    out = dict(envs=N_ENVS, steps=T, minibatch_rows=N_ENVS * T // 4, updates_per_mode=args.rounds * args.updates,
               update_graph=forms,
               update_ms={m: dict(mean=sum(v) / len(v), min_round=min(v), max_round=max(v),
                                  rounds=[round(x, 4) for x in v]) for m, v in per_round.items()})
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
