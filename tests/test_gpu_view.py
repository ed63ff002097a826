"""The follow-camera view on the GPU: hg_view_shapes and hg_render_view (env.view_shapes,
env.render_view) against the independent float64 reference of tests/view_ref.py, and play.py's
recording built on them.

Acceptance rule (tests/test_view_cases.py derives the constants and checks the reference alone
against the rule's conditions): every pixel is sampled at its centre and its four (+-0.01, +-0.01)
pixel corners; depth passes when min t_k - SLACK <= d <= max t_k + SLACK and the id when it is one
of the five ids, both at every pixel; colour is compared, +-1 per channel against the float64 shade
at the centre, at the pixels whose five samples agree on the id (terrain: also on checker square
and triangle).  SLACK is 8 x the reference's float32 replay deviation: 5.0e-6 m on the plane scenes,
6.2e-4 m on the heightfield scenes; the pose pass's bound, 8.8e-5, is 8 x the float32 replay of the
oracle's forward kinematics on the planted poses (one of them 180 m out).
"""
import os

import numpy as np
import pytest
import torch

import depth_ref as DR
import view_ref as VR
from test_gpu_parity import _make_env, _need_gpu
from test_view_cases import FIELD_SLACK, FK_BOUND, SLACK, align_quats, field_scenes, planted

pytestmark = pytest.mark.gpu

f32 = np.float32
BASE_BOX_ID = 2 + 10


def _g(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _plant(env, roots, q):
    """Planted root_states through hg_set_root_state, dof_pos through the view."""
    from humanoid import _native as N
    full = env.root_states.clone().contiguous()
    full[:len(roots)] = torch.from_numpy(np.asarray(roots, f32)).to(full.device)
    N.check(N.lib().hg_set_root_state(env.sim, N.ptr(full), N.stream_ptr(env.device)), env.sim)
    env.dof_pos[:len(q)] = torch.from_numpy(np.asarray(q, f32)).to(full.device)
    torch.cuda.synchronize()


def _render(env, cam, env_ids=None):
    d, i, c = env.render_view(env_ids=env_ids, cam=VR.native_cam(cam), want=("depth", "ids", "rgb"))
    return _g(d), _g(i), _g(c)


def _assert_rule(label, ref, d, i, c, slack):
    ex = np.maximum(np.maximum(ref["lo"] - d, d - ref["hi"]), 0.0)
    fails = VR.failures(ref, d, i, c, slack)
    print(f"{label}: largest depth excess over [lo, hi] {ex.max():.3e} m (slack {slack:.1e}), failures (depth, id, "
          f"colour) {fails}, decided {ref['decided'].mean():.2%}")
    assert fails == (0, 0, 0), label


@pytest.fixture(scope="module")
def model():
    from humanoid import _native as N
    return N.load_model()[0]


@pytest.fixture(scope="module")
def plane_env():
    _need_gpu()
    return _make_env(3)


@pytest.fixture(scope="module")
def field_world(model):
    """The 3-env heightfield env (base depth camera on, so that its buffer exists), the planted field
    states and the reference scene."""
    _need_gpu()
    sc, roots, q, cams = field_scenes(model)
    env = _make_env(3, terrain__mesh_type="heightfield", depth__use_camera=True, depth__original=(16, 12))
    assert np.array_equal(_g(env.height_samples), sc.hf)  # the reference reads the field the GPU reads
    return dict(env=env, sc=sc, roots=roots, q=q, cams=cams)


def test_pose_pass(plane_env, model):
    """view_shapes for the planted envs (default pose; tilted knee bend; joint limits 180 m out)."""
    roots, q = planted(model)
    _plant(plane_env, roots, q)
    got = _g(plane_env.view_shapes())
    want = VR.table_array(VR.world_shapes(model, roots, q, np.float64))
    assert got.shape == (3, 11, 16)
    assert np.array_equal(got[..., 0], want[..., 0])
    got = align_quats(got, want)
    dev = np.abs(got - want).max(axis=(1, 2))
    print(f"pose pass: largest deviation per env {dev} (bound {FK_BOUND:.2e})")
    assert (dev <= FK_BOUND).all()
    assert np.all(got[..., 11:] == 0)
    # env_ids selects rows
    sub = _g(plane_env.view_shapes([2, 0]))
    assert np.array_equal(sub, _g(plane_env.view_shapes())[[2, 0]])


_PLANE_NAMES = [name for name, _, _ in VR.plane_scenes(np.zeros((3, 13)))]


@pytest.mark.parametrize("k", range(len(_PLANE_NAMES)), ids=_PLANE_NAMES)
def test_plane_scenes(plane_env, model, k):
    """Default pose and knee bend on the plane under world cameras in front, to the side, above and low
    (looking up past the robot at the sky)."""
    roots, q = planted(model)
    _plant(plane_env, roots, q)
    name, e, cam = VR.plane_scenes(roots)[k]
    sh = VR.world_shapes(model, roots, q, np.float64)
    ref = VR.reference(DR.scene(None), cam, [sh[e]], [roots[e, :3]])
    d, i, c = _render(plane_env, cam, [e])
    assert (i >= 2).any() and (name.startswith("low") or (i == 1).any())
    if name.startswith("low"):
        assert (i == 0).mean() > 0.5 and (d[i == 0] == f32(cam.far)).all()
        assert (c[i == 0] == np.array(VR.SKY_U8, np.uint8)).all()
    _assert_rule(name, ref, d, i, c, SLACK)


def test_heightfield_follow_camera(field_world, model):
    w = field_world
    _plant(w["env"], w["roots"], w["q"])
    sh = VR.world_shapes(model, w["roots"], w["q"], np.float64)
    for name, cam in w["cams"]:
        ref = VR.reference(w["sc"], cam, sh, w["roots"][:, :3])
        d, i, c = _render(w["env"], cam, list(range(len(w["roots"]))))
        assert (i >= 2).mean() > 0.3 and (i == 1).mean() > 0.3
        _assert_rule(name, ref, d, i, c, FIELD_SLACK)


def test_reset_env_is_drawn_in_its_new_pose(plane_env, model):
    """HG_T_RIGID_STATE keeps the pre-reset pose until the next K_step; the view must not."""
    env = plane_env
    roots, q = planted(model)
    roots[1, :2] += 4.0                                            # well away from where a reset puts it
    _plant(env, roots, q)
    for _ in range(3):
        env.step(torch.zeros(3, 12, device=env.device))
    before = dict(rigid=_g(env.rigid_state)[1:2].astype(np.float64))   # the pose K_step last wrote
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device=env.device)
    env._launch_reset(mask)
    root1, q1 = _g(env.root_states)[1], _g(env.dof_pos)[1]
    assert np.abs(root1[:3] - before["rigid"][0, 0, :3]).max() > 1.0   # the reset moved the robot
    assert np.array_equal(_g(env.rigid_state)[1:2].astype(np.float64), before["rigid"])  # ... and this is stale
    found = VR.decided_camera(DR.scene(None), VR.world_shapes(model, root1[None], q1[None], np.float64), root1)
    assert found is not None, "no camera keeps the reset pose's image within the undecided cap"
    cam, new = found
    d, i, c = _render(env, cam, [1])
    _assert_rule("after the reset", new, d, i, c, SLACK)
    stale = VR.world_shapes(model, root1[None], q1[None], np.float64, rigid=before["rigid"])
    old = VR.reference(DR.scene(None), cam, stale, [root1[:3]])
    fails = VR.failures(old, d, i, c, SLACK)
    print(f"against the pre-reset rigid_state pose: failures {fails}")
    assert fails[0] > 0 and fails[1] > 0                          # the test can tell the difference


def test_env_ids_select_rows(plane_env, model):
    roots, q = planted(model)
    _plant(plane_env, roots, q)
    cam = VR.camera(20, 12, 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0, 1)
    full = _render(plane_env, cam)
    assert full[0].shape == (3, 12, 20) and full[2].shape == (3, 12, 20, 3)
    assert all((full[1][e] >= 2).any() for e in range(3))          # every env's camera sees its robot
    sub = _render(plane_env, cam, [2, 0])
    one = _render(plane_env, cam, torch.tensor([1], device=plane_env.device))
    for a, b, o in zip(full, sub, one):
        assert np.array_equal(b, a[[2, 0]])
        assert np.array_equal(o, a[[1]])
    # one output at a time, into given tensors
    ids = torch.zeros(3, 12, 20, dtype=torch.uint8, device=plane_env.device)
    got = plane_env.render_view(cam=VR.native_cam(cam), ids=ids, want=("ids",))
    assert got is ids and np.array_equal(_g(ids), full[1])
    from humanoid import _native as N
    bad = N.view_cam((20, 12), 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0)
    bad.far_clip = 0.0
    with pytest.raises(ValueError):
        plane_env.render_view(cam=bad)
    import ctypes
    assert N.lib().hg_render_view(plane_env.sim, ctypes.byref(bad), None, 3, N.ptr(ids), None, None,
                                  N.stream_ptr(plane_env.device)) == 1
    assert b"far_clip" in N.lib().hg_last_error(plane_env.sim)
    good = VR.native_cam(cam)
    assert N.lib().hg_render_view(plane_env.sim, ctypes.byref(good), None, 3, None, None, None,
                                  N.stream_ptr(plane_env.device)) == 1
    assert N.lib().hg_render_view(plane_env.sim, ctypes.byref(good), None, 4, N.ptr(ids), None, None,
                                  N.stream_ptr(plane_env.device)) == 1


def test_eye_inside_the_base_box(plane_env, model):
    roots, q = planted(model)
    _plant(plane_env, roots, q)
    cam = VR.camera(9, 7, 60.0, (0.0, 0.0, 0.1), (1.0, 0.2, 0.1), 50.0, 1)
    d, i, c = _render(plane_env, cam)
    assert (d == 0.0).all() and (i == BASE_BOX_ID).all()


def test_camera_outside_the_field_and_below_the_terrain(field_world, model):
    w = field_world
    _plant(w["env"], w["roots"], w["q"])
    sc = w["sc"]
    cam = VR.outside_camera(sc, float(w["roots"][0, 1]))
    sh = VR.world_shapes(model, w["roots"][:1], w["q"][:1], np.float64)
    ref = VR.reference(sc, cam, sh, w["roots"][:1, :3])
    d, i, c = _render(w["env"], cam, [0])
    assert (i == 1).any()                                           # rays enter the extent and hit from below
    _assert_rule("outside and below", ref, d, i, c, FIELD_SLACK)


def test_deterministic_and_read_only(field_world):
    env = field_world["env"]
    _plant(env, field_world["roots"], field_world["q"])
    env.step(torch.zeros(3, 12, device=env.device))
    keep = {k: _g(getattr(env, k)) for k in ("root_states", "dof_pos", "dof_vel", "rigid_state", "depth_buffer")}
    cam = VR.camera(20, 12, 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0, 1)
    a = _render(env, cam)
    b = _render(env, cam)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for k, v in keep.items():
        assert np.array_equal(_g(getattr(env, k)), v), k


def test_graph_capture(plane_env, model):
    """No host synchronisation and no allocation inside the call: it captures and replays."""
    env = plane_env
    roots, q = planted(model)
    _plant(env, roots, q)
    cam = VR.native_cam(VR.camera(20, 12, 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0, 1))
    eager_rgb, eager_d = (t.clone() for t in env.render_view(cam=cam, want=("rgb", "depth")))
    rgb, d = torch.full_like(eager_rgb, 7), torch.full_like(eager_d, -7.0)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        env.render_view(cam=cam, rgb=rgb, depth=d, want=("rgb", "depth"))   # warm-up on the side stream
        stream.synchronize()
        rgb.fill_(7)
        d.fill_(-7.0)
        with torch.cuda.graph(graph, stream=stream):
            env.render_view(cam=cam, rgb=rgb, depth=d, want=("rgb", "depth"))
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert bool((rgb == 7).all()) and bool((d == -7.0).all())   # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(rgb, eager_rgb) and torch.equal(d, eager_d)


def test_play_records_frames(tmp_path, monkeypatch):
    """play(..., record=dir) for 5 steps: 5 PNGs of viewer.record_size that decode, differ, and show
    the robot's colours in their centre region."""
    _need_gpu()
    import sys
    import humanoid.scripts.play as play_mod
    from humanoid.envs import XBotLCfg, XBotLCfgPPO  # noqa: F401  (registers humanoid_ppo)
    from humanoid.utils import get_args, task_registry
    from humanoid.utils.png import read_png
    tr_mod = sys.modules["humanoid.utils.task_registry"]
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.setattr(play_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    args = get_args(["--num_envs", "64", "--headless", "--run_name", "p"])
    env, _ = task_registry.make_env("humanoid_ppo", args=args)
    _, tcfg = task_registry.get_cfgs("humanoid_ppo")
    tcfg.runner.num_steps_per_env = 8
    runner, tcfg = task_registry.make_alg_runner(env, args=args, train_cfg=tcfg)
    runner.learn(1, init_at_random_ep_len=True)
    del runner, env
    torch.cuda.synchronize()
    out = tmp_path / "frames"
    play_mod.play(get_args(["--task", "humanoid_ppo", "--headless"]), steps=5, record=str(out))
    names = sorted(n for n in os.listdir(out) if n.endswith(".png"))
    assert names == ["frame_%05d.png" % k for k in range(5)]
    frames = [read_png(str(out / n)) for n in names]
    W, H = XBotLCfg.viewer.record_size
    assert all(f.shape == (H, W, 3) and f.dtype == np.uint8 for f in frames)
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])
    for f in frames:
        mid = f[H // 4:3 * H // 4, W // 4:3 * W // 4].reshape(-1, 3).astype(np.float64)
        r, g, b = mid[:, 0], mid[:, 1], mid[:, 2]
        # shaded albedos keep their channel ratios (+-1 of rounding on channels >= 60)
        capsule = (r >= 60) & (np.abs(g / r - 0.45 / 0.85) < 0.03) & (np.abs(b / r - 0.15 / 0.85) < 0.03)
        base = (b >= 60) & (np.abs(r / b - 0.25 / 0.70) < 0.03) & (np.abs(g / b - 0.35 / 0.70) < 0.03)
        assert capsule.mean() > 0.005 and base.mean() > 0.005, (capsule.mean(), base.mean())
