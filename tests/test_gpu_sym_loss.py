"""The mirror-symmetry loss on the device: the kernels of csrc/hg_sym.hip against numpy, XBot-L's
observation table against the env's own observation of mirrored states, and the fused, graphed
update with sym_loss=True against the reference's PPO.update (ppo.py:144-226; goldens
ppo_update_sym_{config1,full}.npz from tests/golden/gen_ppo_sym.py).

Tolerances.  hg_sym_loss against float64 numpy on the same float32 inputs: 2^-22 relative — one
rounding each for the difference (2^-24 of d, twice that of d^2), the constant and the product /
the final cast.  The update: test_gpu_ppo_full._compare's rule and constants, unchanged; the
returned symmetry loss within max(1e-4 |ref|, 4 |sym_loss - sym_loss_f64|) — the project's loss
tolerance, or four times the reference's own f32-f64 gap as the generator recorded it.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import test_gpu_ppo_full as F
from test_gpu_ppo_full import R, _compare, _load_storage, _restore

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"config1": ("ppo_update_sym_config1", R.CONFIG1_ENVS), "full": ("ppo_update_sym_full", R.N_ENVS)}
EPS22 = 2.0 ** -22


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def load_split(name):
    """A golden written by gen_ppo_sym.save_split: NAME.npz + NAME.<k>.npz row blocks."""
    main = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    out = {k: main[k] for k in main.files if k != "parts"}
    blocks = {}
    for i in range(int(main["parts"])):
        part = np.load(os.path.join(GOLDEN, f"{name}.{i}.npz"), allow_pickle=False)
        for k in part.files:
            key, r0 = k.rsplit("@", 1)
            blocks.setdefault(key, []).append((int(r0), part[k]))
    for key, bl in blocks.items():
        out[key] = np.concatenate([b for _, b in sorted(bl, key=lambda t: t[0])], axis=0)
    return out


def _tables():
    from humanoid.utils import symmetry as S
    return S.xbotl_mirror()


# ----------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 24, 257])
def test_mirror_rows_shipped_table(rows):
    _need_gpu()
    from humanoid.algo.ppo import hg_sym
    from humanoid.utils import symmetry as S
    stack = S.stack_table(_tables()[0], 15)
    perm, sign = hg_sym.device_table(stack, "cuda:0")
    p, s = S.table_arrays(stack)
    x = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, 705)).astype(np.float32)).cuda()
    out = hg_sym.mirror_rows(x, perm, sign)
    np.testing.assert_array_equal(out.cpu().numpy(), s * x.cpu().numpy()[:, p])


def test_mirror_rows_strided_views():
    """A width-5 hand table; source a column-offset view of a wider table, destination rows wider
    than the row: only the destination's own columns are written."""
    _need_gpu()
    from humanoid.algo.ppo import hg_sym
    table = [3, -0.0001, -4, 1, -2]
    perm, sign = hg_sym.device_table(table, "cuda:0")
    p, s = np.array([3, 0, 4, 1, 2]), np.array([1, -1, -1, 1, -1], np.float32)
    big = torch.from_numpy(np.random.default_rng(3).standard_normal((24, 11)).astype(np.float32)).cuda()
    src = big[:, 4:9]
    dst_big = torch.full((24, 9), 7.0, device="cuda:0")
    out = hg_sym.mirror_rows(src, perm, sign, out=dst_big[:, 2:7])
    assert out.data_ptr() == dst_big[:, 2:7].data_ptr()
    got = dst_big.cpu().numpy()
    np.testing.assert_array_equal(got[:, 2:7], s * big.cpu().numpy()[:, 4:9][:, p])
    assert (got[:, :2] == 7.0).all() and (got[:, 7:] == 7.0).all()


def _sym_ref(mu, mir, p, s, coef):
    mu, mir = mu.astype(np.float64), mir.astype(np.float64)
    d = mu - s * mir[:, p]
    n = d.size
    sym = (d * d).mean()
    g_mu = coef * 2.0 * d / n
    g_mir = np.zeros_like(d)
    g_mir[:, p] = -s * g_mu
    return sym, coef * sym, g_mu, g_mir


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("rows", [1, 7, 24, 1000])
def test_sym_loss_against_float64(rows, coef):
    _need_gpu()
    from humanoid.algo.ppo import hg_sym
    from humanoid.utils import symmetry as S
    act = _tables()[1]
    perm, sign = hg_sym.device_table(act, "cuda:0")
    p, s = S.table_arrays(act)
    rng = np.random.default_rng(100 + rows)
    mu_np = rng.standard_normal((rows, 12)).astype(np.float32)
    mir_np = rng.standard_normal((rows, 12)).astype(np.float32)
    sym_r, loss_r, g_mu_r, g_mir_r = _sym_ref(mu_np, mir_np, p, s.astype(np.float64), coef)
    runs = []
    for _ in range(2):
        mu = torch.from_numpy(mu_np).cuda().requires_grad_()
        mir = torch.from_numpy(mir_np).cuda().requires_grad_()
        loss, sym = hg_sym.sym_loss(mu, mir, perm, sign, coef)
        loss.backward()
        runs.append([t.detach().cpu().numpy() for t in (sym, loss, mu.grad, mir.grad)])
    sym_g, loss_g, g_mu, g_mir = runs[0]
    print(f"rows {rows} coef {coef}: sym rel {abs(sym_g - sym_r) / sym_r:.3g} loss rel "
          f"{abs(loss_g - loss_r) / loss_r:.3g} grad rel max "
          f"{(np.abs(g_mu - g_mu_r) / np.abs(g_mu_r)).max():.3g} {(np.abs(g_mir - g_mir_r) / np.abs(g_mir_r)).max():.3g}")
    assert abs(float(sym_g) - sym_r) <= EPS22 * sym_r
    assert abs(float(loss_g) - loss_r) <= EPS22 * loss_r
    assert (np.abs(g_mu - g_mu_r) <= EPS22 * np.abs(g_mu_r)).all()
    assert (np.abs(g_mir - g_mir_r) <= EPS22 * np.abs(g_mir_r)).all()
    for a, b in zip(*runs):  # a fixed-order float64 reduction: the same bits
        np.testing.assert_array_equal(a, b)
    # a non-unit seed scales both gradients (hg_sym_loss_backward)
    mu = torch.from_numpy(mu_np).cuda().requires_grad_()
    mir = torch.from_numpy(mir_np).cuda().requires_grad_()
    loss, _ = hg_sym.sym_loss(mu, mir, perm, sign, coef)
    loss.backward(gradient=torch.tensor(-2.5, device="cuda:0"))
    np.testing.assert_array_equal(mu.grad.cpu().numpy(), np.float32(-2.5) * g_mu)
    np.testing.assert_array_equal(mir.grad.cpu().numpy(), np.float32(-2.5) * g_mir)


def test_sym_loss_strided_inputs():
    """mu / mu_mirror as column slices of wider tables (row strides above A)."""
    _need_gpu()
    from humanoid.algo.ppo import hg_sym
    from humanoid.utils import symmetry as S
    act = _tables()[1]
    perm, sign = hg_sym.device_table(act, "cuda:0")
    p, s = S.table_arrays(act)
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((70, 20)).astype(np.float32), rng.standard_normal((70, 17)).astype(np.float32)
    loss, sym = hg_sym.sym_loss(torch.from_numpy(a).cuda()[:, 3:15], torch.from_numpy(b).cuda()[:, 5:17], perm, sign)
    sym_r = _sym_ref(a[:, 3:15], b[:, 5:17], p, s.astype(np.float64), 1.0)[0]
    assert abs(float(sym) - sym_r) <= EPS22 * sym_r and float(loss) == float(sym)


# ----------------------------------------------------------------------------------------------
# the observation table against the env's own observation
# ----------------------------------------------------------------------------------------------
def test_obs_table_against_env_observation():
    """Envs 8..15 hold the mirrored state of envs 0..7 (mirror_state, mirrored actions and
    commands, the gait clock half a cycle on): after one post launch their newest observation frame
    is the 47-table applied to that of envs 0..7."""
    _need_gpu()
    from test_gpu_parity import _make_env
    from humanoid import _native as N
    from humanoid.utils import symmetry as S
    env = _make_env(16, noise__add_noise=False, domain_rand__push_robots=False, commands__heading_command=False)
    js = N.load_model()[1]
    limits = np.array(N.model_names(js)[3])
    rng = np.random.default_rng(21)
    q = rng.uniform(limits[:, 0], limits[:, 1], size=(8, 12))
    qd = 0.5 * rng.standard_normal((8, 12))
    root = np.zeros((8, 13))
    root[:, :3] = [0.0, 0.0, 0.95] + 0.1 * rng.standard_normal((8, 3))
    rpy = 0.3 * rng.standard_normal((8, 3))  # tilted roots: xyzw quaternion of roll, pitch, yaw
    cr, sr, cp, sp, cy, sy = (f(rpy[:, i] / 2) for i in range(3) for f in (np.cos, np.sin))
    root[:, 3:7] = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                             cr * cp * cy + sr * sp * sy], axis=1)
    root[:, 7:13] = 0.4 * rng.standard_normal((8, 6))
    act = 0.5 * rng.standard_normal((8, 12))
    cmd = np.concatenate([rng.uniform(0.3, 0.6, (8, 1)), rng.uniform(-0.3, 0.3, (8, 2))], axis=1)
    m_root, m_q, m_qd = S.mirror_state(root, q, qd)
    m_act = act[:, S.JOINT_PERM] * S.JOINT_SIGN
    m_cmd = cmd * np.array([1.0, -1.0, -1.0])
    dev = "cuda:0"
    f32 = lambda a, b: torch.tensor(np.concatenate([a, b]), dtype=torch.float32, device=dev)  # noqa: E731
    L, s = N.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    roots, qs, qds = f32(root, m_root), f32(q, m_q), f32(qd, m_qd)
    ids = torch.arange(16, dtype=torch.int32, device=dev)
    N.check(L.hg_set_root_state(env.sim, ctypes.c_void_p(roots.data_ptr()), s), env.sim)
    N.check(L.hg_set_dof_state_indexed(env.sim, ctypes.c_void_p(ids.data_ptr()), 16, ctypes.c_void_p(qs.data_ptr()),
                                       ctypes.c_void_p(qds.data_ptr()), s), env.sim)
    env.actions[:] = f32(act, m_act)
    env.commands[:, :3] = f32(cmd, m_cmd)
    # half a gait cycle apart (cycle_time 0.64 s / dt 0.01 s = 64 steps), clear of 0, the command
    # resample interval (800) and the time-out (2400)
    assert abs(env.cfg.rewards.cycle_time / env.dt - 64) < 1e-9
    env.episode_length_buf[:8] = torch.arange(100, 108, device=dev)
    env.episode_length_buf[8:] = torch.arange(132, 140, device=dev)
    torch.cuda.synchronize()
    N.check(L.hg_post(env.sim, ctypes.c_uint64(env.common_step_counter + 1), s), env.sim)
    torch.cuda.synchronize()
    assert not env.reset_buf.any()
    frames = env.obs_buf[:, -47:].cpu().numpy().astype(np.float64)
    perm, sign = S.table_arrays(_tables()[0])
    want, got = sign * frames[:8][:, perm], frames[8:]
    assert np.abs(frames[:8]).max(axis=0).min() > 0, "a column of the frame is identically zero: nothing checked"
    err = np.abs(got - want)
    print("phase columns max", err[:, :2].max(), "other columns max rel", (err[:, 2:] / (1 + np.abs(want[:, 2:]))).max())
    assert (err[:, :2] <= 1e-5).all()  # sin(x + pi) in f32 is not exactly -sin x
    assert (err[:, 2:] <= 2e-6 * (1 + np.abs(want[:, 2:]))).all()


# ----------------------------------------------------------------------------------------------
# the update
# ----------------------------------------------------------------------------------------------
def _setup(monkeypatch, case, obs_table=None, **ppo_kw):
    """test_gpu_ppo_full._setup with the symmetry loss on."""
    _need_gpu()
    from humanoid.algo.ppo import ActorCritic, PPO
    n_envs = CASES[case][1]
    obs_perm, act_perm = _tables()
    torch.manual_seed(0)
    ac = ActorCritic(**R.DIMS)
    shapes = [(k, tuple(v.shape)) for k, v in ac.state_dict().items()]
    init = R.parameters(shapes)
    ac.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    kw = dict(R.PPO_KW, sym_loss=True, sym_coef=1.0, obs_permutation=obs_table or obs_perm,
              act_permutation=act_perm, frame_stack=15)
    kw.update(ppo_kw)
    ppo = PPO(ac, device="cuda:0", **kw)
    ppo.init_storage(n_envs, R.T, [R.DIMS["num_actor_obs"]], [R.DIMS["num_critic_obs"]], [R.DIMS["num_actions"]])
    real = torch.randperm

    def randperm_cpu(n, *a, out=None, device=None, **kw):
        # the reference draws the permutation on the CPU generator (storage on the CPU there)
        p = real(n)
        if out is not None:
            out.copy_(p)
            return out
        return p.to(device or "cpu")
    monkeypatch.setattr(torch, "randperm", randperm_cpu)
    return ac, ppo, init


@pytest.fixture(scope="module")
def inputs():
    cache = {}

    def get(case, std):
        if case not in cache:
            cache[case] = R.storage(std, CASES[case][1])
        return cache[case]
    return get


@pytest.fixture(scope="module")
def goldens():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = load_split(CASES[case][0])
        return cache[case]
    return get


def _sym_ok(got, g):
    ref = float(g["sym_loss"])
    tol = max(1e-4 * abs(ref), 4.0 * abs(ref - float(g["sym_loss_f64"])))
    print("sym_loss", float(got), "golden", ref, "tolerance", tol)
    return abs(float(got) - ref) <= tol


@pytest.mark.parametrize("case", list(CASES))
def test_sym_update_eager_matches_reference(monkeypatch, inputs, goldens, case):
    """The first update(): eager, on the fused loss, the mirror gather and the symmetry kernels."""
    ac, ppo, init = _setup(monkeypatch, case)
    g = goldens(case)
    assert ppo._fused_loss and ppo._sym_fused
    _load_storage(ppo, inputs(case, init["std"]))
    torch.manual_seed(R.PERM_SEED)
    losses = ppo.update()
    assert ppo._graphs is None
    fails, _ = _compare(ac, losses, ppo.learning_rate, g, init)
    assert not fails, "; ".join(fails)
    assert _sym_ok(losses[2], g)


@pytest.mark.parametrize("case", list(CASES))
def test_sym_update_graphed_matches_reference(monkeypatch, inputs, goldens, case):
    """The second update(): the whole update, with the mirror, the second actor pass and the
    symmetry loss, replayed from one captured graph."""
    ac, ppo, init = _setup(monkeypatch, case)
    g = goldens(case)
    data = inputs(case, init["std"])
    _load_storage(ppo, data)
    torch.manual_seed(R.PERM_SEED)
    ppo.update()
    _restore(ppo, init)
    _load_storage(ppo, data)
    torch.manual_seed(R.PERM_SEED)
    losses = ppo.update()
    assert ppo._graphs is not None and ppo._graphs[1] is None, "expected the one-graph update"
    assert ppo.update_graph == "one"
    fails, _ = _compare(ac, losses, ppo.learning_rate, g, init)
    assert not fails, "; ".join(fails)
    assert _sym_ok(losses[2], g)
    # sync=False: the symmetry loss stays on the device, a 0-d tensor
    _restore(ppo, init)
    _load_storage(ppo, data)
    torch.manual_seed(R.PERM_SEED)
    dev_losses = ppo.update(sync=False)
    assert torch.is_tensor(dev_losses[2]) and dev_losses[2].dim() == 0 and dev_losses[2].is_cuda
    assert float(dev_losses[2]) == losses[2]


def test_sym_update_detects_missing_term_and_wrong_sign(monkeypatch, inputs, goldens):
    """Sensitivity (config 1): the update without the symmetry term (sym_coef = 0), and with the
    sign of observation-table column 3 flipped, must each FAIL the golden comparison."""
    g = goldens("config1")
    flipped = list(_tables()[0])
    flipped[3] = -flipped[3]
    for kw in (dict(sym_coef=0.0), dict(obs_table=flipped)):
        ac, ppo, init = _setup(monkeypatch, "config1", **kw)
        assert ppo._sym_fused
        _load_storage(ppo, inputs("config1", init["std"]))
        torch.manual_seed(R.PERM_SEED)
        losses = ppo.update()
        fails, _ = _compare(ac, losses, ppo.learning_rate, g, init)
        assert fails, f"{kw}: went undetected by the golden comparison"


def test_sym_update_matches_op_by_op_at_production_size(monkeypatch, inputs):
    """The in-build yardstick: on the full-recipe inputs the new path agrees with the op-by-op
    expression (use_fused_loss=False: the dense mirror products, eager) under _compare's rule, the
    op-by-op result standing in for the golden."""
    ac0, ppo0, init = _setup(monkeypatch, "full")
    ppo0.use_fused_loss = False
    assert not ppo0._fused_loss
    data = inputs("full", init["std"])
    _load_storage(ppo0, data)
    torch.manual_seed(R.PERM_SEED)
    v, s, sym0, lv = ppo0.update()
    assert ppo0.update_graph == "eager"
    ref = dict(value_loss=v, surrogate_loss=s, lin_vel_loss=lv, learning_rate=ppo0.learning_rate)
    ref.update({"final/" + k: t.detach().cpu().numpy() for k, t in ac0.state_dict().items()})
    ac, ppo, _ = _setup(monkeypatch, "full")
    _load_storage(ppo, data)
    torch.manual_seed(R.PERM_SEED)
    losses = ppo.update()
    fails, _ = _compare(ac, losses, ppo.learning_rate, ref, init)
    assert not fails, "; ".join(fails)
    sym0 = float(sym0.detach())
    assert abs(losses[2] - sym0) <= 1e-4 * abs(sym0)


# ----------------------------------------------------------------------------------------------
# the runner
# ----------------------------------------------------------------------------------------------
def test_runner_with_sym_loss(tmp_path):
    _need_gpu()
    from test_gpu_parity import _make_env
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.algo.ppo.on_policy_runner import _JsonlWriter
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = 8
    tcfg.algorithm.sym_loss = True
    train_cfg = class_to_dict(tcfg)
    assert train_cfg["algorithm"]["obs_permutation"] is None
    log_dir = str(tmp_path / "run")
    runner = OnPolicyRunner(_make_env(64), train_cfg, log_dir=log_dir, device="cuda:0")
    assert train_cfg["algorithm"]["obs_permutation"] is None, "the runner works on a copy of the algorithm config"
    assert runner.alg.sym_loss and runner.alg._sym_fused and runner.alg_cfg["frame_stack"] == 15
    runner.writer = _JsonlWriter(log_dir)
    runner.learn(2)
    assert runner.alg.update_graph == "one"
    runner.learn(1)
    rows = [json.loads(ln) for ln in open(os.path.join(log_dir, "scalars.jsonl"))]
    vals = [r["value"] for r in rows if r["tag"] == "Loss/sym_loss"]
    assert len(vals) == 3 and all(math.isfinite(v) and v > 0 for v in vals), vals
    assert runner.last_iteration_stats["sym_loss"] == vals[-1]
    off = XBotLCfgPPO()
    off.runner.num_steps_per_env = 8
    runner2 = OnPolicyRunner(_make_env(64), class_to_dict(off), log_dir=None, device="cuda:0")
    runner2.learn(2)
    assert "sym_loss" not in runner2.last_iteration_stats and runner2.alg.update_graph == "one"
