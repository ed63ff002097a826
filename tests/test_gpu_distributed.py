"""Data parallel on the device, the code the multi-GPU bench runs:

  * sharded envs: two shards [0, n) and [n, 2n) of a 2n-env job step bit-identically to the
    single 2n-env instance (every env draw and the plane / terrain origins are functions of the
    global env id);
  * the PPO update with world_size 2: two ranks share cuda:0 and exchange over gloo (RCCL cannot
    put two ranks on one device); each holds half of the batch and runs the captured two-graph
    minibatch path (backward graph -> all-reduce of the flat gradient + KL slot -> step graph),
    hg_gae with the all-reduced advantage statistics, the fused loss and the fused Adam.  Parameters
    must be bit-identical across ranks and equal to one process updating the concatenated batch
    (world_size 1, its one-graph update) under the same minibatch composition, to the stated fp32
    tolerance (per-minibatch means summed in another order).
"""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _env(n, offset, total, **over):
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.utils.helpers import SimParams
    cfg = XBotLCfg()
    cfg.env.num_envs = n
    cfg.env.env_offset = offset
    cfg.env.num_envs_total = total
    cfg.seed = 11
    cfg.terrain.seed = 5
    for k, v in over.items():
        sec, name = k.split("__")
        setattr(getattr(cfg, sec), name, v)
    return XBotLFreeEnv(cfg, SimParams(), "hg_sim", "cuda:0", True)


_STATE = ("root_states", "dof_pos", "dof_vel", "commands", "env_origins", "env_frictions", "body_mass",
          "rand_push_force", "rand_push_torque", "feet_air_time", "last_actions", "ref_dof_pos", "base_euler_xyz")


@pytest.mark.parametrize("terrain", ["plane", "heightfield"])
def test_sharded_envs_equal_single_instance(terrain):
    """Short episodes (resets), frequent command resamples and pushes, so every Philox purpose is
    drawn; obs noise on.  Bit-identical, env by env."""
    _need_gpu()
    n = 32
    over = dict(terrain__mesh_type=terrain, env__episode_length_s=0.25, commands__resampling_time=0.1,
                domain_rand__push_interval_s=0.15)
    whole = _env(2 * n, 0, 2 * n, **over)
    shards = [_env(n, r * n, 2 * n, **over) for r in range(2)]
    g = torch.Generator(device="cpu").manual_seed(3)
    for step in range(60):
        a = (torch.randn(2 * n, 12, generator=g) * 2.0).to("cuda:0")
        ow, pw, rw, dw, _ = whole.step(a)
        outs = [s.step(a[r * n:(r + 1) * n].contiguous()) for r, s in enumerate(shards)]
        torch.cuda.synchronize()
        for name, x_w, xs in (("obs", ow, [o[0] for o in outs]), ("priv", pw, [o[1] for o in outs]),
                              ("rew", rw, [o[2] for o in outs]), ("reset", dw, [o[3] for o in outs])):
            assert torch.equal(x_w, torch.cat(xs)), f"{name} differs at step {step}"
        for k in _STATE:
            assert torch.equal(getattr(whole, k), torch.cat([getattr(s, k) for s in shards])), f"{k} at step {step}"
    dim = list(whole._sums.shape).index(2 * n)
    assert torch.equal(whole._sums, torch.cat([s._sums for s in shards], dim=dim))


@pytest.mark.parametrize("terrain", ["plane", "heightfield"])
def test_ragged_shards_equal_single_instance(terrain, monkeypatch):
    """Ragged env counts against the well-tested geometry: one 128-env instance and three shards
    of 13, 77 and 38 envs (global ids [0, 13), [13, 90), [90, 128)) step bit-identically, env for
    env, over 40 steps with K_step's wave balancing on (its default).  13 envs: 7 pairs, fewer
    than the 8 XCDs, odd (the last wave's second half is invalid), one partial K_post block; 77
    envs: 39 pairs in XCD ranges of 5 and 4, odd, 5 K_post blocks with 13 envs in the last, an odd
    offset; 38 envs: even, 6 envs in the last K_post block.  Short episodes, frequent resamples
    and pushes, noise on, as in test_sharded_envs_equal_single_instance; every shard resets, its
    last env included.  A wave writing another wave's env, or an env no wave ran, breaks the
    equality: the whole instance cannot share the shards' index slip."""
    _need_gpu()
    monkeypatch.delenv("HG_WAVE_BALANCE", raising=False)
    total, sizes, offs = 128, (13, 77, 38), (0, 13, 90)
    over = dict(terrain__mesh_type=terrain, env__episode_length_s=0.25, commands__resampling_time=0.1,
                domain_rand__push_interval_s=0.15)
    whole = _env(total, 0, total, **over)
    shards = [_env(n, o, total, **over) for n, o in zip(sizes, offs)]
    fields = _STATE + ("torques", "contact_forces", "rigid_state", "rows_dropped", "nonfinite_count", "time_out_buf",
                       "_sums")

    g = torch.Generator(device="cpu").manual_seed(3)
    resets = [torch.zeros(n, dtype=torch.bool, device="cuda:0") for n in sizes]
    for step in range(40):
        a = (torch.randn(total, 12, generator=g) * 2.0).to("cuda:0")
        ow, pw, rw, dw, _ = whole.step(a)
        outs = [s.step(a[o:o + n].contiguous()) for s, n, o in zip(shards, sizes, offs)]
        torch.cuda.synchronize()
        for name, x_w, xs in (("obs", ow, [o[0] for o in outs]), ("priv", pw, [o[1] for o in outs]),
                              ("rew", rw, [o[2] for o in outs]), ("reset", dw, [o[3] for o in outs])):
            assert torch.equal(x_w, torch.cat(xs)), f"{name} differs at step {step}"
        for k in fields:
            parts = torch.cat([getattr(s, k) for s in shards], dim=1 if k == "_sums" else 0)  # _sums is [22, N]
            assert torch.equal(getattr(whole, k), parts), f"{k} at step {step}"
        for r, o in zip(resets, outs):
            r |= o[3]
    for r, n in zip(resets, sizes):
        assert r.any() and bool(r[n - 1]), f"shard of {n} envs: resets {int(r.sum())}, last env {bool(r[n - 1])}"


# ------------------------------------------------------------------------------------------------
# config 4 (BASELINE configs[3]: 32768 envs = 8 x 4096 on the heightfield with DR, one rank per GPU)
# at its per-rank workload on one GPU

C4_RANKS, C4_ENVS = 8, 4096


def test_config4_rank7_shard_contact_parity():
    """Rank 7 of config 4: envs [28672, 32768) of a 32768-env job, heightfield + creation-time DR,
    every draw keyed by the global env id.  After touchdown, one K_step against the C reference
    physics at the stated tolerance on a contact step (>= 95 % of envs on the ground, >= 10 % on a
    sloped triangle, rows dropped equal), then K_post against the pipeline oracle keyed by the same
    global ids (forced resets, timeouts, command resample and a push)."""
    _need_gpu()
    from test_gpu_parity import TOUCHDOWN_STEPS, _assert_contact_step, _post_parity, _step_parity
    r = C4_RANKS - 1
    env = _env(C4_ENVS, r * C4_ENVS, C4_RANKS * C4_ENVS, terrain__mesh_type="heightfield")
    assert env._hgcfg.env_offset == r * C4_ENVS and env._hgcfg.terrain_type == 1
    torch.manual_seed(7)
    for _ in range(TOUCHDOWN_STEPS):
        env.step(torch.randn(env.num_envs, 12, device="cuda:0") * 0.3)
    fr = env.env_frictions.cpu().numpy()
    assert fr.min() >= 0.1 and fr.max() <= 2.0 and fr.std() > 0.3   # DR on: frictions drawn per env
    r64 = _step_parity(env, 173)
    _assert_contact_step(env, r64, sloped_min=0.10)
    _post_parity(env, steps=0)


def test_config4_eight_shards_equal_one_instance():
    """The config-4 split on one GPU: eight shard instances of 4096 envs (env_offset 4096 r,
    num_envs_total 32768) step bit-identically to ONE 32768-env instance, env for env, over 40
    policy steps with resets (2 s episodes cut to 0.3 s), command resamples and pushes every 0.2 s,
    on the heightfield with DR and observation noise: observations, privileged observations,
    rewards, dones and the full state after every step."""
    _need_gpu()
    over = dict(terrain__mesh_type="heightfield", env__episode_length_s=0.3, commands__resampling_time=0.1,
                domain_rand__push_interval_s=0.2)
    n, R = C4_ENVS, C4_RANKS
    whole = _env(R * n, 0, R * n, **over)
    shards = [_env(n, r * n, R * n, **over) for r in range(R)]
    g = torch.Generator(device="cpu").manual_seed(4)
    resets = 0
    for step in range(40):
        a = (torch.randn(R * n, 12, generator=g) * 0.5).to("cuda:0")
        ow, pw, rw, dw, _ = whole.step(a)
        outs = [s.step(a[r * n:(r + 1) * n].contiguous()) for r, s in enumerate(shards)]
        resets += int(dw.sum().item())
        for name, x_w, xs in (("obs", ow, [o[0] for o in outs]), ("priv", pw, [o[1] for o in outs]),
                              ("rew", rw, [o[2] for o in outs]), ("reset", dw, [o[3] for o in outs])):
            assert torch.equal(x_w, torch.cat(xs)), f"{name} differs at step {step}"
        for k in _STATE:
            assert torch.equal(getattr(whole, k), torch.cat([getattr(s, k) for s in shards])), f"{k} at step {step}"
    assert resets >= R * n, resets  # every env went through at least one reset on average
    dim = list(whole._sums.shape).index(R * n)
    assert torch.equal(whole._sums, torch.cat([s._sums for s in shards], dim=dim))
    assert torch.equal(whole.rows_dropped, torch.cat([s.rows_dropped for s in shards]))


# ------------------------------------------------------------------------------------------------
# world_size 2 update vs the single process on the concatenated batch

T_STEPS, N_LOCAL, WORLD = 24, 64, 2


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _perm_sequence(k, size):
    return torch.from_numpy(np.random.RandomState(1000 + k).permutation(size).astype(np.int64))


def _global_batch():
    """Synthetic rollout of WORLD * N_LOCAL envs x T steps (fixed seed)."""
    rs = np.random.RandomState(7)
    n = WORLD * N_LOCAL
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    return dict(observations=f(T_STEPS, n, 705), privileged_observations=f(T_STEPS, n, 219),
                actions=f(T_STEPS, n, 12), rewards=0.1 * f(T_STEPS, n, 1), values=f(T_STEPS, n, 1),
                actions_log_prob=-10.0 + f(T_STEPS, n, 1), mu=0.5 * f(T_STEPS, n, 12),
                sigma=np.full((T_STEPS, n, 12), 1.0, np.float32),
                dones=(rs.uniform(size=(T_STEPS, n, 1)) < 0.05).astype(np.uint8), last_critic=f(n, 219))


def _worker(rank, world, port, out_path, rccl=False):
    """world > 1: rank of a gloo group on cuda:0; world == 1: the single process on everything;
    rccl: the single process in a world-size-1 RCCL ("nccl") group with HG_DP_FORCE=1, i.e. the
    multi-rank update (flat gradient, two graphs per minibatch, all-reduce between them) on RCCL."""
    import sys
    for p in (os.path.join(REPO, "humanoid-gym-with-comments_amd"), REPO):
        sys.path.insert(0, p)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if world > 1 or rccl:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif rccl:
        os.environ["HG_DP_FORCE"] = "1"
        # "eager": the default two-graph form with the eager all-reduce between the replays;
        # "graph": the opt-in one-graph form with the collective captured; "capture_fails": the
        # opt-in form whose capture of the collective raises -> the in-process fallback
        os.environ["HG_DP_GRAPH_COLLECTIVE"] = "0" if rccl == "eager" else "1"
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        assert dist.get_backend() == "nccl"
        if rccl == "capture_fails":
            real_all_reduce = dist.all_reduce

            def all_reduce(t, *a, **k):
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("injected: the collective refuses stream capture")
                return real_all_reduce(t, *a, **k)
            dist.all_reduce = all_reduce
    import bench
    from humanoid.algo.ppo import ActorCritic, PPO
    dev = "cuda:0"
    tc = bench.train_cfg(T_STEPS)
    torch.manual_seed(0)
    ac = ActorCritic(705, 219, 12, **tc["policy"]).to(dev)
    ppo = PPO(ac, device=dev, **tc["algorithm"])
    n = N_LOCAL if world > 1 else WORLD * N_LOCAL
    ppo.init_storage(n, T_STEPS, [705], [219], [12])
    G = _global_batch()
    sl = slice(rank * N_LOCAL, (rank + 1) * N_LOCAL) if world > 1 else slice(None)
    st = ppo.storage
    # minibatch composition: one local permutation p_k per update call on every rank; the single
    # process's minibatch i is the union of the ranks' minibatches i
    calls = [0]
    real_randperm = torch.randperm

    def randperm(size, *args, out=None, device=None, **kw):
        k = calls[0]
        calls[0] += 1
        if world > 1:
            idx = _perm_sequence(k, size)
        else:
            nmb = ppo.num_mini_batches
            B = size // WORLD
            mbl = B // nmb
            p = _perm_sequence(k, B)
            parts = []
            for i in range(nmb):
                for r in range(WORLD):
                    b = p[i * mbl:(i + 1) * mbl]
                    t, el = b // N_LOCAL, b % N_LOCAL
                    parts.append(t * (WORLD * N_LOCAL) + r * N_LOCAL + el)
            idx = torch.cat(parts)
        idx = idx.to(device if device is not None else "cpu")
        if out is not None:
            out.copy_(idx)
            return out
        return idx
    torch.randperm = randperm
    import warnings
    try:
        losses = []
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            _updates(ppo, st, G, sl, dev, losses)
        torch.cuda.synchronize()
    finally:
        torch.randperm = real_randperm
    flat = torch.cat([p.detach().reshape(-1) for p in ac.parameters()]).cpu()
    torch.save({"flat": flat, "lr": float(ppo.learning_rate), "losses": losses, "graphed": ppo._graphs is not None,
                "whole": bool(getattr(ppo, "_whole", False)), "calls": calls[0], "dp": bool(ppo._dp),
                "update_graph": ppo.update_graph, "capture_error": ppo.capture_error,
                "collectives": ppo.collectives_per_update(),
                "backend": dist.get_backend() if dist.is_initialized() else None,
                "accumulate_grad_warnings": sum("AccumulateGrad" in str(w.message) for w in caught)}, out_path)
    if dist.is_initialized():
        dist.destroy_process_group()


def _updates(ppo, st, G, sl, dev, losses):
    for _ in range(3):  # eager warm-up, capture + replay, replay
        for k in ("observations", "privileged_observations", "actions", "rewards", "values", "actions_log_prob",
                  "mu", "sigma", "dones"):
            getattr(st, k).copy_(torch.from_numpy(G[k][:, sl]).to(dev))
        st.step = T_STEPS
        ppo.compute_returns(torch.from_numpy(G["last_critic"][sl]).to(dev))
        losses.append(ppo.update())


def test_dp_graphed_update_matches_single_process(tmp_path):
    _need_gpu()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, str(tmp_path / f"rank{r}.pt"))) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
        assert p.exitcode == 0, f"rank process exit code {p.exitcode}"
    single = ctx.Process(target=_worker, args=(0, 1, 0, str(tmp_path / "single.pt")))
    single.start()
    single.join(240)
    assert single.exitcode == 0
    R = [torch.load(tmp_path / f"rank{r}.pt", weights_only=True) for r in range(WORLD)]
    S = torch.load(tmp_path / "single.pt", weights_only=True)
    assert all(r["graphed"] and not r["whole"] for r in R), "ranks must run the two-graph all-reduce path"
    assert S["graphed"] and S["whole"]
    assert R[0]["calls"] == S["calls"] == 3
    assert all(x["accumulate_grad_warnings"] == 0 for x in R + [S])
    # ranks: bit-identical parameters and learning rate
    for r in R[1:]:
        assert torch.equal(r["flat"], R[0]["flat"])
        assert r["lr"] == R[0]["lr"]
    # vs the single process: same learning-rate decisions, parameters within the stated tolerance
    assert R[0]["lr"] == S["lr"]
    d = (R[0]["flat"] - S["flat"]).abs()
    print(f"dp vs single: max |dparam| {d.max().item():.3e}, lr {S['lr']:.3e}, "
          f"losses dp {R[0]['losses'][-1]} single {S['losses'][-1]}")
    # 3 updates x 2 epochs x 4 minibatches of Adam steps at lr <= 1e-5 * 1.5^k: a parameter moves by
    # at most ~lr per step; reassociated fp32 means agree to ~1e-6 relative, so the parameters agree
    # far inside one step
    assert d.max().item() <= 1e-6
    # the loss means a rank reports are over its own rows; their average over the ranks is the
    # single process's mean over all rows
    for i, b in enumerate(S["losses"][-1]):
        a = sum(float(r["losses"][-1][i]) for r in R) / WORLD
        assert abs(a - float(b)) <= 1e-5 * max(1.0, abs(float(b)))


@pytest.mark.parametrize("mode", ["graph", "eager", "capture_fails"])
def test_rccl_update_matches_single_process(tmp_path, mode):
    """The RCCL code path executed: a world-size-1 "nccl" group with the multi-rank update forced
    (HG_DP_FORCE=1) — parameter broadcast, the flat gradient buffer with the KL slot, the
    advantage-statistics all-reduce, and per minibatch backward -> all_reduce on RCCL -> step:
    mode "eager" is the default two-graph form with the all-reduce between the replays; mode
    "graph" (HG_DP_GRAPH_COLLECTIVE=1) captures the collective inside the ONE update graph; mode
    "capture_fails" is that opt-in with the collective raising under capture:
    the update must fall back in the same process to the two-graph form and say so.  At world
    size 1 the all-reduce is the identity, so the parameters must equal the single-process
    update bit for bit in every mode."""
    _need_gpu()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    runs = {}
    for name, rccl in (("rccl", mode), ("single", False)):
        p = ctx.Process(target=_worker, args=(0, 1, _port(), str(tmp_path / f"{name}.pt"), rccl))
        p.start()
        p.join(240)
        assert p.exitcode == 0, f"{name} process exit code {p.exitcode}"
        runs[name] = torch.load(tmp_path / f"{name}.pt", weights_only=True)
    R, S = runs["rccl"], runs["single"]
    assert R["backend"] == "nccl" and R["dp"] and R["graphed"] and R["whole"] == (mode == "graph")
    assert R["update_graph"] == ("one" if mode == "graph" else "two")
    assert (R["capture_error"] is not None) == (mode == "capture_fails"), R["capture_error"]
    assert R["collectives"] == 2 * 4 + 1 and S["collectives"] == 0 and S["update_graph"] == "one"
    assert S["backend"] is None and not S["dp"] and S["whole"]
    assert R["calls"] == S["calls"] == 3
    assert R["lr"] == S["lr"]
    assert torch.equal(R["flat"], S["flat"]), f"max |d| {(R['flat'] - S['flat']).abs().max().item():.3e}"
    for a, b in zip(R["losses"], S["losses"]):
        assert [float(x) for x in a] == [float(x) for x in b]
