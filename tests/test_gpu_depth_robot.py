"""The depth camera with the robot's own legs in view, on the GPU: hg_render_depth_robot
(depth.draw_robot, env.render_depth(draw_robot=...)) against the combined float64 reference of
tests/depth_robot_ref.py, and the env surface around it.

Acceptance rule (tests/test_depth_robot_cases.py derives the constant and checks the reference alone
against the rule's conditions): a pixel d passes when lo - SLACK <= d <= hi + SLACK, [lo, hi]
spanning the reference at the pixel centre and its four (+-0.01, +-0.01) pixel corners; no pixel is
excluded.  SLACK = 8 x the reference's own float32 replay deviation (3.1e-5 m) = 2.5e-4 m.
"""
import ctypes

import numpy as np
import pytest
import torch

import depth_ref as DR
import depth_robot_ref as RR
import view_ref as VR
from test_depth_robot_cases import SLACK
from test_gpu_parity import _make_env, _need_gpu
from test_gpu_view import _plant

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -7.0


def _g(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


@pytest.fixture(scope="module")
def model():
    from humanoid import _native as N
    return N.load_model()[0]


def _env(size, **over):
    _need_gpu()
    return _make_env(3, depth__use_camera=True, depth__draw_robot=True, depth__original=size, depth__normalize=False, **over)


@pytest.fixture(scope="module")
def world(model):
    """The three 3-env envs of the scene set (plane at 17 x 9 and 16 x 12, heightfield at 17 x 9), their
    planted states and a cache of references (each computed once)."""
    plane = DR.scene(None)
    roots, q, pitch = RR.plane_set(model)
    sc, fr, fq, fp = RR.field_set(model)
    images = {}
    for size in RR.PLANE_SIZES:
        images["plane %dx%d" % size] = dict(env=_env(size), sc=plane, cam=RR.camera(size), roots=roots, q=q, pitch=pitch)
    field = _env(RR.FIELD_SIZE, terrain__mesh_type="heightfield")
    assert np.array_equal(_g(field.height_samples), sc.hf)  # the reference reads the field the GPU reads
    images["field %dx%d" % RR.FIELD_SIZE] = dict(env=field, sc=sc, cam=RR.camera(RR.FIELD_SIZE), roots=fr, q=fq, pitch=fp)
    cache = {}

    def ref(label):
        if label not in cache:
            w = images[label]
            cache[label] = RR.reference(w["sc"], w["cam"], model, w["roots"], w["q"], w["pitch"])
        return cache[label]
    return dict(images=images, ref=ref)


def _set(env, roots, q, pitch):
    _plant(env, roots, q)
    env.depth_cam_pitch[:len(pitch)] = torch.from_numpy(np.asarray(pitch, f32)).to(env.device)
    torch.cuda.synchronize()


def _plant_image(w):
    _set(w["env"], w["roots"], w["q"], w["pitch"])
    return w["env"], len(w["roots"])


def _raw_terrain_only(env):
    """hg_render_depth itself, with the env's camera."""
    from humanoid import _native as N
    cam = N.depth_cam(env._depth)
    out = torch.full((env.num_envs, cam.height, cam.width), SENTINEL, device=env.device)
    N.check(N.lib().hg_render_depth(env.sim, ctypes.byref(cam), N.ptr(env.depth_cam_pitch), N.ptr(out),
                                    ctypes.c_int64(cam.height * cam.width), ctypes.c_uint64(env.common_step_counter),
                                    N.stream_ptr(env.device)), env.sim)
    return out


LABELS = ["plane %dx%d" % s for s in RR.PLANE_SIZES] + ["field %dx%d" % RR.FIELD_SIZE]


@pytest.mark.parametrize("label", LABELS)
def test_scene_set(world, label):
    """Default pose, tilted knee bend and joint limits 180 m out under cameras pitched 60, 75 and 45
    degrees: every pixel of every image inside its interval."""
    env, n = _plant_image(world["images"][label])
    ref = world["ref"](label)
    d = _g(env.render_depth())[:n]
    ex = np.maximum(np.maximum(ref["lo"] - d, d - ref["hi"]), 0.0)
    bad = RR.failures(ref, d, SLACK)
    print(f"{label}: largest excess over [lo, hi] per env {ex.max(axis=(1, 2))} m (slack {SLACK:.1e}), pixels outside "
          f"{bad.sum()}, robot pixels {ref['robot'].all(0).sum(axis=(1, 2))}")
    assert not bad.any(), (label, np.argwhere(bad)[:5].tolist())


@pytest.mark.parametrize("label", LABELS)
def test_option_off_is_hg_render_depth(world, label):
    """draw_robot=False on the same env is hg_render_depth bit for bit, and that frame fails the rule at
    a robot pixel of every image: the rule can tell the difference."""
    env, n = _plant_image(world["images"][label])
    ref = world["ref"](label)
    off = env.render_depth(draw_robot=False)
    assert torch.equal(off, _raw_terrain_only(env))
    bad = RR.failures(ref, _g(off)[:n], SLACK) & ref["robot"].all(0)
    print(f"{label}: terrain-only frame fails at {bad.sum(axis=(1, 2))} robot pixels per env")
    assert (bad.sum(axis=(1, 2)) >= 1).all()
    assert not torch.equal(env.render_depth(), off)


def test_hands_and_base_box_are_not_drawn(world, model):
    """Default pose under a camera looking straight down, 16 x 12 (the CPU test's image)."""
    w = world["images"]["plane 16x12"]
    pitch = np.array([RR.HANDS_PITCH])
    _set(w["env"], w["roots"], w["q"], pitch)
    real = RR.reference(w["sc"], w["cam"], model, w["roots"][:1], w["q"][:1], pitch)
    loc = VR.local_shapes(model)
    hands = [k for k, s in enumerate(loc) if s[0] == VR.CAPSULE and s[1] == 0]
    with_hands = RR.reference(w["sc"], w["cam"], model, w["roots"][:1], w["q"][:1], pitch, select=RR.drawn(model) + hands)
    d = _g(w["env"].render_depth())[:1]
    assert not RR.failures(real, d, SLACK).any()
    assert RR.failures(with_hands, d, SLACK).sum() >= 1
    assert d.min() > 0.3            # the base box, which contains the camera, would give 0 everywhere
    assert real["robot"].all(0).sum() >= 1


def test_reset_env_is_drawn_in_its_new_pose(world, model):
    """HG_T_RIGID_STATE keeps the pre-reset pose until the next K_step; the depth image must not."""
    w = world["images"]["plane 16x12"]
    env = w["env"]
    roots = w["roots"].copy()
    roots[1, :2] += 4.0                                            # well away from where a reset puts it
    _set(env, roots, w["q"], w["pitch"])
    for _ in range(3):
        env.step(torch.zeros(3, 12, device=env.device))
    before = _g(env.rigid_state)[1:2].astype(np.float64)           # the pose K_step last wrote
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device=env.device)
    env._launch_reset(mask)
    root1, q1, pitch1 = _g(env.root_states)[1:2], _g(env.dof_pos)[1:2], _g(env.depth_cam_pitch)[1:2]
    assert np.abs(root1[0, :3] - before[0, 0, :3]).max() > 1.0     # the reset moved the robot
    assert np.array_equal(_g(env.rigid_state)[1:2].astype(np.float64), before)   # ... and this is stale
    d = _g(env.render_depth())[1:2]
    new = RR.reference(w["sc"], w["cam"], model, root1, q1, pitch1)
    assert new["robot"].all(0).sum() >= 3
    assert not RR.failures(new, d, SLACK).any()
    old = RR.reference(w["sc"], w["cam"], model, root1, q1, pitch1, rigid=before)
    fails = RR.failures(old, d, SLACK).sum()
    print(f"against the pre-reset rigid_state pose: {fails} pixels fail")
    assert fails >= 1                                              # the test can tell the difference


@pytest.mark.parametrize("label", LABELS)
def test_post_processing_is_shared(world, label):
    """Noise, clamp and normalisation act on the combined t with hg_render_depth's key: with both on,
    drawing the robot changes no pixel that has no robot sample.  Deterministic and read-only."""
    env, n = _plant_image(world["images"][label])
    ref = world["ref"](label)
    keep = {k: _g(getattr(env, k)) for k in ("root_states", "dof_pos", "rigid_state")}
    on = env.render_depth(normalize=True, noise=0.02, draw_robot=True)
    off = env.render_depth(normalize=True, noise=0.02, draw_robot=False)
    plain = env.render_depth(normalize=True, noise=0.0, draw_robot=False)
    assert not torch.equal(off, plain)                             # the noise is on
    diff = (_g(on) - _g(off))[:n]
    none = ~ref["robot"].any(0)
    assert none.mean() > 0.5 and (diff[none] == 0.0).all()
    legs = diff[ref["robot"].all(0)]
    assert (legs <= 0.0).all() and (legs < 0.0).mean() > 0.9       # a leg is nearer than the ground behind it
    assert float(on.min()) >= -0.5 and float(on.max()) <= 0.5
    assert torch.equal(env.render_depth(normalize=True, noise=0.02, draw_robot=True), on)
    for k, v in keep.items():
        assert np.array_equal(_g(getattr(env, k)), v), k


def test_render_view_shares_the_table_region(world):
    """hg_render_view writes the same arena region; stream order keeps the two calls apart."""
    env, _ = _plant_image(world["images"]["plane 17x9"])
    cam = VR.native_cam(VR.camera(20, 12, 60.0, (2.0, -2.0, 0.8), (0.0, 0.0, -0.2), 50.0, 1))
    d1 = env.render_depth().clone()
    v1 = env.render_view(cam=cam, want=("depth",))[0].clone()
    d2 = env.render_depth().clone()
    v2 = env.render_view(cam=cam, want=("depth",))[0].clone()
    assert torch.equal(d1, d2) and torch.equal(v1, v2)
    assert float(v1.min()) < 50.0 and not torch.equal(d1, env.render_depth(draw_robot=False))


def test_graph_capture(world):
    """No host synchronisation and no allocation inside the call: it captures and replays."""
    env, _ = _plant_image(world["images"]["field 17x9"])
    eager = env.render_depth().clone()
    out = torch.full_like(eager, SENTINEL)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        env.render_depth(out=out)   # warm-up on the side stream
        stream.synchronize()
        out.fill_(SENTINEL)
        with torch.cuda.graph(graph, stream=stream):
            env.render_depth(out=out)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())   # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_step_path(world):
    """env.step() on a render step leaves extras["depth"] equal to render_depth() of the same state,
    legs included."""
    env, _ = _plant_image(world["images"]["plane 16x12"])
    frame = None
    for _ in range(env._depth_interval):
        extras = env.step(torch.zeros(3, 12, device=env.device))[4]
        if extras["depth"] is not None:
            frame = extras["depth"]
            break
    assert frame is not None and frame.data_ptr() == env.depth_frame(0).data_ptr()
    assert torch.equal(frame, env.render_depth())
    assert torch.equal(frame, env.depth_buffer[:, (env._depth_renders - 1) % env._depth_len])
    assert not torch.equal(frame, env.render_depth(draw_robot=False))


def test_refusals_and_config(world):
    from humanoid import _native as N
    env = world["images"]["plane 17x9"]["env"]
    out = torch.full((3, 9, 17), SENTINEL, device=env.device)
    cam = N.depth_cam(env._depth)
    args = lambda c, o, stride: (env.sim, ctypes.byref(c), N.ptr(env.depth_cam_pitch), o, ctypes.c_int64(stride),  # noqa: E731
                                 ctypes.c_uint64(0), N.stream_ptr(env.device))
    assert N.lib().hg_render_depth_robot(*args(cam, N.ptr(out), 152)) == 1
    assert N.lib().hg_last_error(env.sim).startswith(b"hg_render_depth_robot")
    assert N.lib().hg_render_depth_robot(*args(cam, None, 153)) == 1
    bad = N.depth_cam(env._depth)
    bad.far_clip = 0.0
    assert N.lib().hg_render_depth_robot(*args(bad, N.ptr(out), 153)) == 1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert N.lib().hg_render_depth_robot(*args(cam, N.ptr(out), 153)) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
    with pytest.raises(ValueError):
        _make_env(3, depth__draw_robot=True)   # without depth.use_camera
