"""Measured terrain heights in the privileged frame (terrain.critic_heights, BUILD-DEFINED;
include/hgsim.h hg_cfg.critic_heights) on the GPU: the window kernel's height columns against the
float32 replay `expected_height_columns` (tests/test_critic_heights_cfg.py, pinned there to the
reference's own heights), evaluated on the GPU's own post-launch root states; columns 0..72 against
oracle/pipeline_ref.post fed the 73-column slices of the history; stacking, reset and window wraps
over the full row width; the default-off identity; the ABI's refusals; the critic MLP and the
trainer at the new widths.

Height columns: at least 99.9 % of entries bitwise equal and every entry within scale * 0.1, the
cap and bound tests/test_gpu_parity.py::test_measured_heights uses (a float tie on a cell boundary
in the yaw rotation moves a sample to the neighbouring cell)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from test_critic_heights_cfg import expected_height_columns
from test_gpu_parity import _make_env, _need_gpu, _oracle_cfg, _post_once, snapshot

pytestmark = pytest.mark.gpu

f32 = np.float32
W0 = 73                                   # the privileged frame's own columns
GRID_3X3 = dict(terrain__measured_points_x=[-0.6, 0.0, 0.6], terrain__measured_points_y=[-0.4, 0.0, 0.4])


def _g(t):
    return t.detach().cpu().numpy().copy()


def _heights_env(n, grid="default", **over):
    kw = dict(terrain__mesh_type="heightfield", terrain__critic_heights=True)
    if grid == "3x3":
        kw.update(GRID_3X3)
    kw.update(over)
    env = _make_env(n, **kw)
    P = 9 if grid == "3x3" else 187
    assert env._hgcfg.critic_heights == P and env._priv_width == W0 + P
    return env, P


def _frames(stack, W):
    """[N, F * W] stack -> [N, F, W]."""
    return stack.reshape(stack.shape[0], -1, W)


def _expect(env, root=None):
    """The helper on the env's grid and heightfield, at `root` (default: the GPU's root states now)."""
    hf = _g(env.height_samples) if getattr(env, "height_samples", None) is not None else None
    root = _g(env.root_states) if root is None else root
    return expected_height_columns(_oracle_cfg(env), root, _g(env._critic_height_xy), hf)


def _assert_height_columns(got, want, scale, label=""):
    exact = float((got == want).mean())
    worst = float(np.abs(got - want).max())
    print(f"height columns {label}: {exact:.5f} of {got.size} entries bitwise equal, max |d| {worst:.3g} "
          f"(bound {scale * 0.1:.3g})")
    assert got.shape == want.shape
    assert exact >= 0.999, (label, exact)
    assert worst <= scale * 0.1, (label, worst)


def _steps(env, k, seed, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    for _ in range(k):
        env.step((torch.randn(env.num_envs, 12, generator=g) * scale).to("cuda:0"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("grid", ["default", "3x3"])
@pytest.mark.parametrize("n", [64, 77])
def test_frame_parity(n, grid):
    """One post launch after 30 seeded steps with envs 0..15 terminated (terrain curriculum on: they
    move to other sub-terrains): columns 0..72 of the newest frame and of the stack against
    pipeline_ref.post at _post_parity's tolerances, the height columns against the helper at the
    GPU's post-launch pose; the history's height columns shifted / zeroed with the rest."""
    import pipeline_ref as PR
    _need_gpu()
    env, P = _heights_env(n, grid, terrain__curriculum=True)
    W = W0 + P
    assert env._hgcfg.curriculum == 1 and env.num_privileged_obs == 3 * W
    assert env.cfg.env.num_privileged_obs == 3 * W and env.cfg.env.single_num_privileged_obs == W
    _steps(env, 30, 1000 + n)
    m = 16
    env.contact_forces[0:m, 0, 2] = 50.0                           # terminate envs 0..15
    env.root_states[0:4, 0] = env.env_origins[0:4, 0] + 5.0         # walked far: level up
    env.root_states[4:8, :2] = env.env_origins[4:8, :2]             # stood still ...
    env.commands[4:8, 0] = 0.5                                      # ... under a command: level down
    counter = 777
    S, hist_o, hist_p = snapshot(env)
    assert hist_p.shape == (n, 3 * W)
    pre_root = S["root_states"].copy()
    prev = _frames(hist_p, W)
    hist_p73 = np.ascontiguousarray(prev[:, :, :W0]).reshape(n, 3 * W0)
    cfg = _oracle_cfg(env)
    obs, priv, rew, reset, timeout, terms = PR.post(cfg, S, counter, hist_o, hist_p73)
    _post_once(env, counter)
    assert reset[:m].all()
    np.testing.assert_array_equal(_g(env.reset_buf), reset)
    np.testing.assert_allclose(_g(env.root_states), S["root_states"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(_g(env.obs_buf), obs, rtol=1e-4, atol=1e-4)
    got = _frames(_g(env.privileged_obs_buf), W)
    assert got.shape == (n, 3, W)
    np.testing.assert_allclose(got[:, :, :W0], _frames(priv, W0), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got[:, 2, :W0], _frames(priv, W0)[:, 2], rtol=1e-4, atol=1e-4)
    scale = float(env._hgcfg.critic_height_scale)
    assert scale == 5.0
    _assert_height_columns(got[:, 2, W0:], _expect(env), scale, f"n={n} P={P}")
    # the older frames over the full width: zeros for the reset envs, the previous stack's newer
    # frames, bit for bit, for the others
    rs = reset.astype(bool)
    assert (got[rs, :2, :] == 0).all()
    np.testing.assert_array_equal(got[~rs, :2, :], prev[~rs, 1:, :])
    # the test can fail (oracle side only): the expectation is neither constant nor clipped away,
    # and the reset envs' pose moved under the grid
    want = expected_height_columns(cfg, S["root_states"], _g(env._critic_height_xy), _g(env.height_samples))
    varied = float((np.ptp(want, axis=1) > 0).mean())
    clipped = float((np.abs(want) == f32(scale)).mean())
    before = expected_height_columns(cfg, pre_root, _g(env._critic_height_xy), _g(env.height_samples))
    moved = float((before[:m] != want[:m]).mean())
    print(f"oracle side n={n} P={P}: {varied:.3f} of envs with non-constant columns, {clipped:.3f} of entries on a "
          f"clip bound, {moved:.3f} of the reset envs' entries differ from the pre-reset pose's")
    assert varied > 0.10 and clipped < 0.50 and moved > 0.10


def test_reset_route():
    """env.reset_idx([3, 5, 40]) (hg_reset_masked): the newest frame's height columns at the
    post-reset pose for every env, the history of exactly those envs zeroed across the full width,
    the other envs' older frames the previous stack's, bit for bit.  (Columns 0..72 through this
    route are held bitwise to the option-off env by test_nothing_else_moves.)"""
    _need_gpu()
    env, P = _heights_env(64)
    W = W0 + P
    _steps(env, 6, 21)
    prev = _frames(_g(env.privileged_obs_buf), W)
    root0 = _g(env.root_states)
    ids = np.array([3, 5, 40])
    env.reset_idx(torch.tensor(ids, device="cuda:0"))
    torch.cuda.synchronize()
    got = _frames(_g(env.privileged_obs_buf), W)
    keep = np.setdiff1d(np.arange(64), ids)
    root1 = _g(env.root_states)
    np.testing.assert_array_equal(root1[keep], root0[keep])
    assert (root1[ids, :3] != root0[ids, :3]).any(axis=1).all()
    assert (got[ids, :2, :] == 0).all()
    np.testing.assert_array_equal(got[keep, :2, :], prev[keep, 1:, :])
    _assert_height_columns(got[:, 2, W0:], _expect(env), 5.0, "reset_idx")
    # unmoved envs, unmoved terrain: their height columns are the previous frame's
    np.testing.assert_array_equal(got[keep, 2, W0:], prev[keep, 2, W0:])
    assert np.isfinite(got).all() and (got[ids, 2, :W0] != 0).any()


def test_window_wraps():
    """3 x 3 grid, 64 envs, past two wraps of the window with forced resets in the middle: at every
    step the stack is the last c_frame_stack newest frames the test recorded, frames from before an
    env's reset zeros, at width 82."""
    _need_gpu()
    env, P = _heights_env(64, "3x3")
    W, F = W0 + P, 3
    assert W == 82
    hw = int(env.hg.hg_obs_window_advance(env.sim))
    first = _frames(env.privileged_obs_buf.clone(), W)
    frames = [first[:, j].clone() for j in range(F)]     # newest frame after each launch so far
    resets = [torch.zeros(64, dtype=torch.bool, device="cuda:0") for _ in range(F)]
    steps = 2 * hw + F + 2
    heads = set()
    g = torch.Generator().manual_seed(9)
    for k in range(steps):
        if k in (hw // 2, hw + 3, 2 * hw - 1):
            env.episode_length_buf[(5 * k) % 60:(5 * k) % 60 + 3] = 2400     # time out on this step
        env.step((torch.randn(64, 12, generator=g) * 0.3).to("cuda:0"))
        heads.add(int(env.hg.hg_obs_head(env.sim)))
        stack = _frames(env.privileged_obs_buf, W)
        assert stack.shape == (64, F, W)
        frames.append(stack[:, F - 1].clone())
        resets.append(env.reset_buf.clone())
        for j in range(F - 1):
            # frame j of the stack was the newest F - 1 - j launches ago; zero if the env reset since
            since = torch.stack(resets[len(resets) - (F - 1 - j):]).any(0)
            want = torch.where(since.view(-1, 1), torch.zeros_like(frames[0]), frames[len(frames) - (F - j)])
            assert torch.equal(stack[:, j], want), (k, j)
    assert 0 in heads and len(heads) == hw
    assert sum(int(r.any()) for r in resets) >= 3
    assert all(bool((f[:, W0:] != 0).any()) for f in frames[F:])


def test_nothing_else_moves():
    """The option off and on, the same seed and the same actions for 30 steps with forced time-outs
    and a reset_idx call: observations, rewards, resets, root / dof state and columns 0..72 of every
    privileged frame are bitwise equal; with the option off the table and the widths are what they
    were (219)."""
    _need_gpu()
    from humanoid import _native as N
    off = _make_env(64, terrain__mesh_type="heightfield", terrain__curriculum=True)
    on, P = _heights_env(64, terrain__curriculum=True)
    W = W0 + P
    hw = int(off.hg.hg_obs_window_advance(off.sim))
    assert off._hgcfg.critic_heights == 0 and not off._hgcfg.critic_height_points
    assert tuple(off._view(N.T["PRIV_BUF"]).shape) == (64, (3 - 1 + hw) * W0)
    assert tuple(on._view(N.T["PRIV_BUF"]).shape) == (64, (3 - 1 + hw) * W)
    assert off.num_privileged_obs == 219 and off.cfg.env.num_privileged_obs == 219
    assert off.cfg.env.single_num_privileged_obs == 73 and off.privileged_obs_buf.shape == (64, 219)
    assert on.num_privileged_obs == 780 and on.privileged_obs_buf.shape == (64, 780)
    g = torch.Generator().manual_seed(4)
    n_reset = 0
    for k in range(30):
        a = (torch.randn(64, 12, generator=g) * 0.4).to("cuda:0")
        for env in (off, on):
            if k in (7, 19):
                env.episode_length_buf[k:k + 5] = 2400
            if k == 12:
                env.reset_idx([3, 5, 40])
            env.step(a.clone())
        torch.cuda.synchronize()
        n_reset += int(off.reset_buf.sum())
        for name in ("obs_buf", "rew_buf", "reset_buf", "root_states", "dof_pos", "dof_vel", "commands",
                     "terrain_levels"):
            assert torch.equal(getattr(off, name), getattr(on, name)), (k, name)
        assert torch.equal(_frames(off.privileged_obs_buf, W0), _frames(on.privileged_obs_buf, W)[:, :, :W0]), k
    assert n_reset >= 10


def test_boundary():
    """hg_create refuses a positive count with a NULL grid and a count over the maximum (nothing is
    created); hg_update_cfg refuses a changed count or grid pointer and accepts a changed scale,
    which the next frame uses; on the plane the columns are clip(z - 0.5, -1, 1) * scale."""
    _need_gpu()
    from humanoid import _native as N
    L = N.lib()
    env, P = _heights_env(64)
    W = W0 + P
    nbytes = L.hg_arena_bytes(ctypes.byref(env._hgcfg))
    arena = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    base = arena.data_ptr() + (-arena.data_ptr()) % 256

    def create(**fields):
        c = N.HgCfg.from_buffer_copy(env._hgcfg)
        for k, v in fields.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        rc = L.hg_create(ctypes.byref(c), ctypes.byref(env._model), ctypes.c_void_p(base), ctypes.c_size_t(nbytes),
                         ctypes.byref(h))
        msg = L.hg_last_error(None).decode() if rc else ""
        if rc == 0:
            L.hg_destroy(h)
        return rc, msg

    rc, msg = create(critic_height_points=None)
    assert rc != 0 and "critic_height_points" in msg
    rc, msg = create(critic_heights=N_MAX + 1)
    assert rc != 0 and "critic_heights" in msg
    rc, msg = create(critic_heights=-1)
    assert rc != 0 and "critic_heights" in msg
    _steps(env, 3, 5)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fields in (dict(critic_heights=P - 1), dict(critic_heights=0),
                   dict(critic_height_points=env._critic_height_xy.data_ptr() + 8)):
        c = N.HgCfg.from_buffer_copy(env._hgcfg)
        for k, v in fields.items():
            setattr(c, k, v)
        assert L.hg_update_cfg(env.sim, ctypes.byref(c), s) != 0, fields
        assert b"layout" in L.hg_last_error(env.sim)
    env._hgcfg.critic_height_scale = 2.5
    N.check(L.hg_update_cfg(env.sim, ctypes.byref(env._hgcfg), s), env.sim)
    _post_once(env, env.common_step_counter + 1)
    got = _frames(_g(env.privileged_obs_buf), W)
    want = _expect(env)
    assert np.abs(want).max() <= 2.5 and np.abs(want).max() > 0.5
    _assert_height_columns(got[:, 2, W0:], want, 2.5, "after hg_update_cfg")
    # the plane
    flat = _make_env(64, terrain__critic_heights=True)
    assert flat._hgcfg.terrain_type == 0 and flat.num_privileged_obs == 780
    _steps(flat, 12, 6)
    got = _frames(_g(flat.privileged_obs_buf), W)
    z = _g(flat.root_states)[:, 2:3]
    want = np.repeat(np.clip(z - f32(0.5), f32(-1), f32(1)) * f32(5.0), P, axis=1)
    np.testing.assert_array_equal(got[:, 2, W0:], want)
    np.testing.assert_array_equal(want, _expect(flat))
    assert np.ptp(z) > 0 and (np.abs(want) < 5.0).any()


N_MAX = 1024  # HG_MAX_HEIGHT_POINTS (include/hgsim.h)


@pytest.mark.parametrize("rows", [96, 4096, 8256])
@pytest.mark.parametrize("K", [780, 246])
def test_critic_mlp_at_the_new_widths(K, rows):
    """The critic MLP's forward and backward at the new first-layer widths (K = 3 * (73 + 187) on
    the routed GEMM, K = 3 * (73 + 9), no multiple of 4, on the fallback) against torch in float64,
    at test_fused_mlp_backward_matches_torch's tolerances; the inference path too.  8256 rows: the
    second tile of the K = 780 forward route and the k_wgrad_tr route of its 768 x 780 weight
    gradient (both start above 8192 rows)."""
    _need_gpu()
    from humanoid.algo.ppo import ActorCritic
    torch.manual_seed(3)
    ac = ActorCritic(705, K, 12, actor_hidden_dims=[512, 256, 128], critic_hidden_dims=[768, 256, 128],
                     base_lin_vel_hidden_dims=[128, 128]).cuda()
    assert ac.critic[0].in_features == K
    ref = copy.deepcopy(ac.critic).double()
    x = torch.randn(rows, K, device="cuda:0")
    w = torch.randn(rows, 1, device="cuda:0")
    ac.fused_mlp = True
    v = ac._mlp(ac.critic, x)
    (v * w).sum().backward()
    v64 = ref(x.double())
    (v64 * w.double()).sum().backward()
    torch.testing.assert_close(v.detach(), v64.detach().float(), rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        torch.testing.assert_close(ac._mlp(ac.critic, x), v64.detach().float(), rtol=1e-5, atol=1e-5)
    for (name, p), q in zip(ac.critic.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.grad, q.grad.float(), rtol=2e-4, atol=2e-5, msg=lambda m: f"{name}: {m}")


@pytest.mark.parametrize("grid", ["default", "3x3"])
def test_through_the_trainer(grid, tmp_path):
    """OnPolicyRunner.learn, 64 envs x 24 steps, two iterations eager then graphed: the critic's first
    layer is 3 * (73 + P) wide, the losses are finite, the critic observations stored for a rollout
    step are the stack the env returned for it, and a checkpoint of another width is refused."""
    _need_gpu()
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    env, P = _heights_env(64, grid)
    K = 3 * (W0 + P)
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = 24
    runner = OnPolicyRunner(env, class_to_dict(tcfg), log_dir=None, device="cuda:0")
    alg = runner.alg
    assert alg.actor_critic.critic[0].in_features == K
    assert tuple(alg.storage.privileged_observations.shape) == (24, 64, K)
    # one rollout step by hand: what PPO.act stores is what the env handed out
    obs, cobs = env.get_observations(), env.get_privileged_observations()
    assert cobs.shape == (64, K) and cobs.data_ptr() == env.privileged_obs_buf.data_ptr()
    seen = cobs.clone()
    with torch.inference_mode():
        a = alg.act(obs, cobs)
        env.episode_length_buf[:8] = int(env.max_episode_length)   # resets rewrite the live window
        _, _, rew, dones, infos = env.step(a)
        alg.process_env_step(rew, dones, infos)
    torch.cuda.synchronize()
    assert dones[:8].all()
    assert torch.equal(alg.storage.privileged_observations[0], seen)
    assert (seen.view(64, 3, -1)[:, 2, W0:] != 0).any()
    alg.storage.clear()
    alg.use_graphs = False
    runner.learn(2)
    st = runner.last_iteration_stats
    assert all(np.isfinite(st[k]) for k in ("value_loss", "surrogate_loss", "lin_vel_loss")), st
    assert alg.update_graph == "eager"
    alg.use_graphs = True
    runner.learn(3)
    st = runner.last_iteration_stats
    assert all(np.isfinite(st[k]) for k in ("value_loss", "surrogate_loss", "lin_vel_loss")), st
    assert alg.update_graph in ("one", "two")
    assert torch.isfinite(env.privileged_obs_buf).all()
    for p in alg.actor_critic.parameters():
        assert torch.isfinite(p).all()
    # a checkpoint of another critic width is refused before any tensor is copied
    path = str(tmp_path / "model.pt")
    runner.save(path)
    other = _make_env(64, terrain__mesh_type="heightfield")
    r2 = OnPolicyRunner(other, class_to_dict(tcfg), log_dir=None, device="cuda:0")
    before = {k: v.clone() for k, v in r2.alg.actor_critic.state_dict().items()}
    with pytest.raises(ValueError) as err:
        r2.load(path)
    assert str(K) in str(err.value) and "219" in str(err.value) and "terrain.critic_heights" in str(err.value)
    for k, v in r2.alg.actor_critic.state_dict().items():
        assert torch.equal(v, before[k]), k
    runner.load(path)  # its own width loads
