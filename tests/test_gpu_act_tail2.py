"""hg_rollout_act_tail2 (the actor's split-K finish, its 512 -> 256 and 256 -> 128 layers, the 12 x 128
head and the sampling in one launch) against the three launches it replaces (hg_gemm_f32_splitk's
finishing launch, hg_gemm_f32 tile 5, hg_rollout_act_tail): every stored array bit for bit; the
route applies exactly where hg_mlp.mlp_infer_tail2 states; a short training run is unchanged; and
hg_gemm_f32_splitk_partials leaves the workspace hg_gemm_f32_splitk leaves."""
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("actions", "actions_log_prob", "mu", "sigma", "observations", "privileged_observations")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _actor_critic(hidden=(512, 256, 128)):
    from humanoid.algo.ppo import ActorCritic
    torch.manual_seed(7)
    return ActorCritic(705, 219, 12, actor_hidden_dims=list(hidden), critic_hidden_dims=[768, 256, 128],
                       init_noise_std=0.8).to("cuda:0")


@pytest.fixture(scope="module")
def ac():
    _need_gpu()
    return _actor_critic()


def _inputs(n):
    g = torch.Generator(device="cuda:0").manual_seed(1000 + n)
    big = torch.randn(n, 705 + 47, device="cuda:0", generator=g)
    return big[:, 47:], torch.randn(n, 219, device="cuda:0", generator=g)  # obs 4 bytes off 16-byte alignment


def _act(ac, obs, cobs, tail2):
    """Slot 0 of a fresh storage after one PPO.act with TAIL2_FUSED = ``tail2``."""
    from humanoid.algo.ppo import PPO, hg_mlp
    n = obs.shape[0]
    keep = hg_mlp.TAIL2_FUSED
    hg_mlp.TAIL2_FUSED = tail2
    try:
        ppo = PPO(ac, device="cuda:0")
        ppo._rollout_seed = 777
        ppo.init_storage(n, 2, [705], [219], [12])
        with torch.inference_mode():
            ppo.act(obs, cobs)
        st = ppo.storage
        return {k: getattr(st, k)[0].clone() for k in KEYS}
    finally:
        hg_mlp.TAIL2_FUSED = keep


def _assert_same(a, b):
    for k in KEYS:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [1, 16, 17, 250, 1000])
def test_tail2_matches_the_three_launches_bitwise(ac, n):
    """One row in a block, one full block, a full block plus a row, ragged counts over several
    blocks: actions, log-probs, mu, sigma and both observation slots equal the split-K finish +
    tile 5 + hg_rollout_act_tail route's, which is the route the tables give at every n here."""
    from humanoid.algo.ppo import hg_mlp
    obs, cobs = _inputs(n)
    W1, b1 = ac.actor[0].weight, ac.actor[0].bias
    assert hg_mlp._gemm_fwd_splitk(obs, W1, b1) == (25, 4)
    assert hg_mlp._route(hg_mlp._GEMM_FWD, n, 512, 256) == 5
    with torch.inference_mode():
        assert hg_mlp.mlp_infer_tail2(ac.actor, obs) is not None  # the fused route is the one taken
    fused, three = _act(ac, obs, cobs, True), _act(ac, obs, cobs, False)
    _assert_same(fused, three)
    with torch.inference_mode():
        torch.testing.assert_close(fused["mu"], ac.actor(obs), rtol=1e-5, atol=1e-5)
    assert torch.equal(fused["observations"], obs) and torch.equal(fused["privileged_observations"], cobs)


def test_tail2_route_applies_where_stated(ac, monkeypatch):
    """Not None for the bench's actor at the bench's row count; None for a host tensor, another
    net shape, another slice count and an unfused tail — and PPO.act then writes the older
    route's bits."""
    from humanoid.algo.ppo import hg_mlp
    obs4k, _ = _inputs(4096)
    obs, cobs = _inputs(250)
    with torch.inference_mode():
        t2 = hg_mlp.mlp_infer_tail2(ac.actor, obs4k)
        assert t2 is not None and t2[0].numel() == 4 * 4096 * 512 and t2[1] == 4
        assert hg_mlp.mlp_infer_tail2(ac.actor, obs.cpu()) is None  # never a host tensor's address
        other = _actor_critic((512, 128, 128))
        assert hg_mlp.mlp_infer_tail2(other.actor, obs) is None
    _assert_same(_act(other, obs, cobs, True), _act(other, obs, cobs, False))
    with monkeypatch.context() as m:  # what HG_SPLITK_ROUTE=25,2 sets at import
        m.setitem(hg_mlp._GEMM_FWD_SPLITK, (705, 512), [(4096, (25, 2))])
        with torch.inference_mode():
            assert hg_mlp.mlp_infer_tail2(ac.actor, obs) is None
        _assert_same(_act(ac, obs, cobs, True), _act(ac, obs, cobs, False))
    with monkeypatch.context() as m:
        m.setattr(hg_mlp, "TAIL_FUSED", False)
        with torch.inference_mode():
            assert hg_mlp.mlp_infer_tail2(ac.actor, obs) is None
        unfused = _act(ac, obs, cobs, True)
        _assert_same(unfused, _act(ac, obs, cobs, False))
    with torch.inference_mode():
        assert hg_mlp.mlp_infer_tail2(ac.actor, obs) is not None
    _assert_same(_act(ac, obs, cobs, True), unfused)  # and the fused launch gives those bits too


def test_learn_is_unchanged_by_tail2(monkeypatch):
    """OnPolicyRunner.learn(2) at 64 envs with the fused launch and with the three launches:
    the same parameters and storage slots bit for bit."""
    _need_gpu()
    from humanoid.envs import XBotLCfg, XBotLCfgPPO
    from humanoid.envs.custom.humanoid_env import XBotLFreeEnv
    from humanoid.algo.ppo import OnPolicyRunner, hg_mlp
    from humanoid.utils.helpers import SimParams, class_to_dict, set_seed
    calls = {True: 0, False: 0}
    real = hg_mlp.mlp_infer_tail2

    def counted(net, x):
        r = real(net, x)
        calls[hg_mlp.TAIL2_FUSED] += r is not None
        return r

    monkeypatch.setattr(hg_mlp, "mlp_infer_tail2", counted)
    runs = []
    for mode in (True, False):
        monkeypatch.setattr(hg_mlp, "TAIL2_FUSED", mode)
        set_seed(11)
        cfg = XBotLCfg()
        cfg.env.num_envs = 64
        cfg.seed = 11
        env = XBotLFreeEnv(cfg, SimParams(), "hg_sim", "cuda:0", True)
        tcfg = XBotLCfgPPO()
        tcfg.runner.num_steps_per_env = 24
        tcfg.seed = 11
        runner = OnPolicyRunner(env, class_to_dict(tcfg), log_dir=None, device="cuda:0")
        runner.learn(2, init_at_random_ep_len=True)
        torch.cuda.synchronize()
        alg, st = runner.alg, runner.alg.storage
        out = {"p%d" % i: p.detach().cpu().clone() for i, p in enumerate(alg.actor_critic.parameters())}
        for k in ("observations", "privileged_observations", "rewards", "dones", "actions", "actions_log_prob", "mu",
                  "sigma", "values", "returns", "advantages"):
            out["st_" + k] = getattr(st, k).detach().cpu().clone()
        runs.append(out)
        del runner, env
        torch.cuda.synchronize()
    assert calls[True] == 2 * 24 and calls[False] == 0  # every collection step took the fused launch, or none
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert torch.isfinite(runs[0][k].double()).all(), k
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("M", [17, 256])
def test_splitk_partials_leave_the_workspace_of_the_full_entry(M):
    """hg_gemm_f32_splitk_partials' slices are the ones hg_gemm_f32_splitk sums: the same
    workspace bit for bit, and summed in slice order + bias (the finishing launch's arithmetic,
    act = 0) they give hg_gemm_f32_splitk's C bit for bit; unaligned rows at M = 17."""
    _need_gpu()
    from humanoid import _native as N
    L = N.lib()
    n, k, tile, S = 512, 705, 25, 4
    g = torch.Generator(device="cuda:0").manual_seed(M)
    x = torch.randn(M, k + 47, device="cuda:0", generator=g)[:, 47:] if M == 17 else \
        torch.randn(M, k, device="cuda:0", generator=g)
    W = torch.randn(n, k, device="cuda:0", generator=g) * 0.05
    b = torch.randn(n, device="cuda:0", generator=g)
    s = torch.cuda.current_stream().cuda_stream
    ws_full = torch.full((S, M, n), float("nan"), device="cuda:0")
    ws_part = torch.full((S, M, n), float("nan"), device="cuda:0")
    C = torch.empty(M, n, device="cuda:0")
    rc = L.hg_gemm_f32_splitk(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), b.data_ptr(), C.data_ptr(), n,
                              ws_full.data_ptr(), ws_full.numel(), M, n, k, 0, tile, S, s)
    assert rc == 0
    rc = L.hg_gemm_f32_splitk_partials(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ws_part.data_ptr(),
                                       ws_part.numel(), M, n, k, tile, S, s)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(ws_part).all()
    assert torch.equal(ws_part, ws_full)
    assert torch.equal(((ws_part[0] + ws_part[1]) + ws_part[2]) + ws_part[3] + b, C)
    # the same refusals as the full entry: a workspace one float short, a slice count that leaves a slice empty
    assert L.hg_gemm_f32_splitk_partials(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ws_part.data_ptr(),
                                         ws_part.numel() - 1, M, n, k, tile, S, s) != 0
    assert L.hg_gemm_f32_splitk_partials(x.data_ptr(), x.stride(0), W.data_ptr(), W.stride(0), ws_part.data_ptr(),
                                         ws_part.numel(), M, n, 40, tile, S, s) != 0
