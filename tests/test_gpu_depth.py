"""The depth camera on the GPU: hg_render_depth against the independent numpy reference
(tests/depth_ref.py: brute-force two-sided Moeller-Trumbore in float64), and the env surface built
on it (depth_buffer ring, depth_frame, render_depth, extras["depth"], shards, graph capture).

Acceptance rule of every geometric comparison (tests/test_depth_ref.py derives the constant): a
pixel d passes when lo - SLACK <= d <= hi + SLACK, [lo, hi] spanning the float64 reference at the
pixel centre and its four (+-0.01, +-0.01) pixel corners; no pixel is excluded.  SLACK = 8 x the
reference's own float32 replay deviation (5.5e-6 m) = 4.4e-5 m.
"""
import ctypes

import numpy as np
import pytest
import torch

import depth_ref as DR
import rng_ref
from test_depth_ref import SLACK
from test_gpu_parity import _make_env, _need_gpu

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = -7.0


def _g(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


@pytest.fixture(scope="module")
def world():
    """The scene set's terrain, the 24-env heightfield env standing on it (camera on, 16 x 12) and a
    cache of reference intervals (each computed once)."""
    _need_gpu()
    hf, origins, tcfg = DR.terrain_field()
    env = _make_env(DR.SCENE_ENVS, terrain__mesh_type="heightfield", depth__use_camera=True, depth__original=(16, 12))
    assert np.array_equal(_g(env.height_samples), hf)  # the reference reads the field the GPU reads
    sc = DR.field_scene(hf, tcfg)
    cache = {}

    def ref(key, cam, roots, pitch):
        if key not in cache:
            cache[key] = DR.intervals(sc, cam, roots, pitch)
        return cache[key]
    return dict(env=env, sc=sc, origins=origins, ref=ref)


def _plant(env, roots, pitch=None):
    """Roots [k, 13] into envs 0 .. k - 1 (hg_set_root_state), their camera pitches into depth_cam_pitch."""
    from humanoid import _native as N
    full = env.root_states.clone().contiguous()
    full[:len(roots)] = torch.from_numpy(np.asarray(roots, f32)).to(full.device)
    N.check(N.lib().hg_set_root_state(env.sim, N.ptr(full), N.stream_ptr(env.device)), env.sim)
    if pitch is not None:
        env.depth_cam_pitch[:len(pitch)] = torch.from_numpy(np.asarray(pitch, f32)).to(full.device)
    torch.cuda.synchronize()


def _cam(W, H, fov=87.0, near=0.0, far=3.0, normalize=0, noise=0.0):
    from humanoid import _native as N
    c = N.HgDepthCam()
    c.width, c.height, c.horizontal_fov_deg = W, H, fov
    c.pos[0], c.pos[1], c.pos[2] = 0.10, 0.0, 0.15
    c.near_clip, c.far_clip, c.normalize, c.noise = near, far, normalize, noise
    return c


def _raw_call(env, cam, out, stride, counter=0, pitch="env", sim="env"):
    from humanoid import _native as N
    p = env.depth_cam_pitch if isinstance(pitch, str) else pitch
    return N.lib().hg_render_depth(env.sim if isinstance(sim, str) else sim, ctypes.byref(cam) if cam is not None else None,
                                   N.ptr(p) if p is not None else None, N.ptr(out) if out is not None else None,
                                   ctypes.c_int64(stride), ctypes.c_uint64(counter), N.stream_ptr(env.device))


def _render(env, cam, counter=0):
    out = torch.full((env.num_envs, cam.height, cam.width), SENTINEL, device=env.device)
    assert _raw_call(env, cam, out, cam.height * cam.width, counter) == 0
    return _g(out)


def _assert_inside(d, lo, hi, label):
    d = np.asarray(d, np.float64)
    assert np.isfinite(d).all(), f"{label}: non-finite pixels"
    ex = np.maximum(np.maximum(lo - d, d - hi), 0.0)
    print(f"{label}: largest excess over [lo, hi] {ex.max():.3e} m (slack {SLACK:.1e}), pixels outside {(ex > 0).sum()}")
    bad = np.argwhere(ex > SLACK)
    assert len(bad) == 0, f"{label}: {len(bad)} pixels outside their interval, first (env, row, col) {bad[0]}, " \
                          f"got {d[tuple(bad[0])]}, interval [{lo[tuple(bad[0])]}, {hi[tuple(bad[0])]}]"


@pytest.mark.parametrize("size", [(16, 12), (13, 7)])
def test_parity_on_the_scene_set(world, size):
    """13 x 7 is no tile multiple and its odd width puts column 6 at u = 0 exactly."""
    env = world["env"]
    roots, pitch = DR.scene_set(world["origins"])
    _plant(env, roots, pitch)
    lo, hi, ctr = world["ref"](("scene", size), DR.camera(*size), roots, pitch)
    d = _render(env, _cam(*size))
    assert (d < 3.0).mean() > 0.3
    _assert_inside(d, lo, hi, f"scene set {size}")


def test_degenerate_rays(world):
    """Centre column parallel to a grid axis (level bases at yaw 0, pi/2, pi, -pi/2, W = 13), and a
    central ray pointing straight down (camera pitch exactly pi/2)."""
    env = world["env"]
    roots, pitch = DR.degenerate_set(world["origins"])
    _plant(env, roots, pitch)
    lo, hi, ctr = world["ref"]("degenerate", DR.camera(13, 7), roots, pitch)
    d = _render(env, _cam(13, 7))[:len(roots)]
    _assert_inside(d, lo, hi, "degenerate rays")
    assert (d[4] < 3.0).all() and (d[:4, -1] < 3.0).all()   # straight down sees ground everywhere


def test_field_extent(world):
    env = world["env"]
    roots, pitch = DR.extent_set(world["sc"], world["origins"])
    _plant(env, roots, pitch)
    lo, hi, ctr = world["ref"]("extent", DR.camera(16, 12), roots, pitch)
    d = _render(env, _cam(16, 12))[:len(roots)]
    _assert_inside(d, lo, hi, "field extent")
    assert (d[0, -1] < 3.0).all() and (d[0, :6] == 3.0).all()   # inside looking out: ground, then nothing
    assert (d[1] < 3.0).mean() > 0.3                            # outside looking in: rays enter and hit
    assert (d[2] < 1.0).all()                                   # under the surface looking up
    assert (d[3] == 3.0).all()                                  # NaN root position: far_clip, and the call returned
    _plant(env, DR.scene_set(world["origins"])[0])


def test_plane_terrain():
    _need_gpu()
    env = _make_env(5, depth__use_camera=True, depth__original=(16, 12))
    roots, pitch = DR.scene_set(np.zeros((20, 20, 3)), n=5)
    _plant(env, roots, pitch)
    want = DR.render(DR.scene(None), DR.camera(16, 12), roots, pitch)[0]
    d = _render(env, _cam(16, 12))
    assert (want < 3.0).mean() > 0.3
    err = np.abs(d - want).max()
    print(f"plane: largest deviation from the analytic depth {err:.3e} m (slack {SLACK:.1e})")
    assert err <= SLACK


def _noise_replay(seed, gid, counter, npix, noise):
    pix = np.arange(npix)
    nblk = (npix + 3) // 4
    words = np.stack(rng_ref.rng4(int(seed), np.full(nblk, gid), counter, np.arange(nblk), 11), axis=1)  # [nblk, 4]
    u = rng_ref.u01(words[pix >> 2, pix & 3])
    return (f32(noise) * (f32(2.0) * u - f32(1.0))).astype(f32)


def _noise_error_ok(noisy, raw, want, inner):
    """noisy - raw equals the replayed noise within 1e-6 — wherever float32 can hold the sum that
    well: the kernel stores round(raw + noise), off by up to half a float32 spacing of the stored
    value, which is below 1e-6 only under 16 m.  Farther pixels (far_clip is 100 m here) are held to
    that half spacing instead; none is left out."""
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(noisy), np.abs(raw)).astype(f32)).astype(np.float64)
    tol = np.maximum(1e-6, 1.01 * half_ulp + 1e-8)
    assert (tol[raw < 16.0] == 1e-6).all()
    err = np.abs((noisy.astype(np.float64) - raw.astype(np.float64)) - want.astype(np.float64))
    print(f"noise replay: largest error {err[inner].max():.3e}, under 16 m {err[inner & (raw < 16.0)].max():.3e}")
    return bool((err <= tol)[inner].all())


def test_clip_normalise_noise(world):
    env = world["env"]
    roots, pitch = DR.scene_set(world["origins"])
    _plant(env, roots, pitch)
    raw = _render(env, _cam(16, 12))
    # normalise, with clips that bite on both sides
    near, far = f32(1.2), f32(2.5)
    assert (raw < near).any() and (raw > far).any()
    clipped = _render(env, _cam(16, 12, near=float(near), far=float(far)))   # the GPU's own raw frame at these clips
    assert np.abs(clipped - np.clip(raw, near, far)).max() <= 1e-5 and clipped.min() == near and clipped.max() == far
    got = _render(env, _cam(16, 12, near=float(near), far=float(far), normalize=1))
    want = ((clipped - near) / (far - near) - f32(0.5)).astype(f32)
    assert (np.abs(got - want) <= np.spacing(np.abs(want)).astype(f32) + f32(6e-8)).all()
    assert got.min() == -0.5 and got.max() == 0.5
    # noise: the Philox words, replayed, at two counters (the second past 2^32)
    raw100 = _render(env, _cam(16, 12, far=100.0))
    for counter in (3, (1 << 33) + 5):
        noisy = _render(env, _cam(16, 12, far=100.0, noise=0.02), counter)
        for e in (0, 7, 23):
            want = _noise_replay(env._hgcfg.seed, e, counter, 192, 0.02).reshape(12, 16)
            inner = (raw100[e] > 0.05) & (raw100[e] < 99.0)   # away from the clips
            assert inner.mean() > 0.3
            assert _noise_error_ok(noisy[e], raw100[e], want, inner)
    assert not np.array_equal(_render(env, _cam(16, 12, far=100.0, noise=0.02), 3), noisy)


@pytest.mark.parametrize("n,mesh", [(5, "heightfield"), (77, "plane")])
def test_env_surface(n, mesh):
    _need_gpu()
    env = _make_env(n, terrain__mesh_type=mesh, depth__use_camera=True, depth__original=(16, 12),
                    depth__update_interval=5, depth__buffer_len=2)
    assert env.depth_buffer.shape == (n, 2, 12, 16) and env.depth_buffer.dtype == torch.float32
    assert env.depth_cam_pitch.shape == (n,) and env.depth_cam_pitch.dtype == torch.float32
    lo, hi = np.deg2rad(20.0), np.deg2rad(30.0)
    p = _g(env.depth_cam_pitch)
    assert (p >= lo - 1e-6).all() and (p <= hi + 1e-6).all() and (n < 2 or p.std() > 0)
    # creation: one render, in every slot
    first = env.render_depth()
    assert torch.equal(env.depth_buffer[:, 0], first) and torch.equal(env.depth_buffer[:, 1], first)
    assert "depth" not in env.extras or env.extras["depth"] is None
    assert float(first.min()) >= -0.5 and float(first.max()) <= 0.5 and float(first.min()) < 0.4   # normalised, not all far
    g = torch.Generator(device="cpu").manual_seed(1)
    kept = {}
    for step in range(1, 13):
        _, _, _, _, extras = env.step((torch.randn(n, 12, generator=g) * 0.3).to("cuda:0"))
        assert env.common_step_counter == step
        if step % 5 == 0:
            frame = extras["depth"]
            assert isinstance(frame, torch.Tensor) and frame.shape == (n, 12, 16)
            assert frame.stride() == (2 * 12 * 16, 16, 1) and frame.data_ptr() == env.depth_frame(0).data_ptr()
            assert torch.equal(frame, env.render_depth())   # the post-reset pose of this step
            kept[step] = frame.clone()
        else:
            assert "depth" in extras and extras["depth"] is None
    assert torch.equal(env.depth_frame(0), kept[10]) and torch.equal(env.depth_frame(1), kept[5])
    assert not torch.equal(kept[10], kept[5])
    with pytest.raises(ValueError):
        env.depth_frame(2)
    # the render of step 15 goes to the older slot only
    env.depth_frame(0).fill_(SENTINEL)
    newest = env.depth_frame(0).data_ptr()
    for step in range(13, 16):
        _, _, _, _, extras = env.step(torch.zeros(n, 12, device="cuda:0"))
    assert extras["depth"].data_ptr() != newest
    assert bool((env.depth_frame(1) == SENTINEL).all()) and not bool((env.depth_frame(0) == SENTINEL).any())
    # on demand, into a given tensor, in metres
    out = torch.full((n, 12, 16), SENTINEL, device="cuda:0")
    assert env.render_depth(out=out, normalize=False) is out
    assert float(out.min()) > 0.0 and float(out.max()) <= 3.0
    want = ((out - 0.0) / 3.0 - 0.5)
    assert float((env.render_depth() - want).abs().max()) <= 1.2e-7
    with pytest.raises(ValueError):
        env.render_depth(out=torch.empty(n, 12, 17, device="cuda:0"))


def test_rendering_does_not_touch_the_sim():
    _need_gpu()
    over = dict(terrain__mesh_type="heightfield", env__episode_length_s=0.05)
    on = _make_env(32, depth__use_camera=True, depth__original=(16, 12), depth__update_interval=2, **over)
    off = _make_env(32, **over)
    for k in ("depth_buffer", "depth_cam_pitch", "depth_frame", "render_depth"):
        assert hasattr(on, k) and not hasattr(off, k), k
    g = torch.Generator(device="cpu").manual_seed(2)
    resets = 0
    for step in range(10):
        a = (torch.randn(32, 12, generator=g) * 0.5).to("cuda:0")
        ra, rb = on.step(a), off.step(a)
        assert "depth" in ra[4] and "depth" not in rb[4]
        resets += int(ra[3].sum())
        for name, x, y in (("obs", ra[0], rb[0]), ("priv", ra[1], rb[1]), ("rew", ra[2], rb[2]), ("reset", ra[3], rb[3]),
                           ("root", on.root_states, off.root_states)):
            assert torch.equal(x, y), f"{name} differs at step {step}"
    assert resets > 0
    assert torch.equal(on.obs_buf, off.obs_buf) and torch.equal(on.privileged_obs_buf, off.privileged_obs_buf)


def test_shards_render_and_draw_like_one_instance():
    """Modelled on test_ragged_shards_equal_single_instance: shards of 13 and 35 envs of a 48-env
    job, noise on, render frames and draw camera pitches bitwise equal to the single instance's rows;
    the noise of a shard env replays from its GLOBAL id."""
    _need_gpu()
    from test_gpu_distributed import _env
    total, sizes, offs = 48, (13, 35), (0, 13)
    over = dict(terrain__mesh_type="heightfield", depth__use_camera=True, depth__original=(16, 12),
                depth__dis_noise=0.02, depth__update_interval=3)
    whole = _env(total, 0, total, **over)
    shards = [_env(n, o, total, **over) for n, o in zip(sizes, offs)]
    assert torch.equal(whole.depth_cam_pitch, torch.cat([s.depth_cam_pitch for s in shards]))
    assert torch.equal(whole.depth_buffer, torch.cat([s.depth_buffer for s in shards]))
    g = torch.Generator(device="cpu").manual_seed(3)
    for step in range(6):
        a = (torch.randn(total, 12, generator=g) * 0.5).to("cuda:0")
        whole.step(a)
        for s, n, o in zip(shards, sizes, offs):
            s.step(a[o:o + n].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(whole.root_states, torch.cat([s.root_states for s in shards]))
    assert torch.equal(whole.depth_buffer, torch.cat([s.depth_buffer for s in shards]))
    assert not torch.equal(whole.depth_frame(0), whole.depth_frame(1))
    # shard 1 (env_offset 13), local env 4 = global env 17, at the counter of the last render
    sh = shards[1]
    assert sh._hgcfg.env_offset == 13 and sh.common_step_counter == 6
    raw = _g(sh.render_depth(normalize=False, noise=0.0))[4]
    noisy = _g(sh.render_depth(normalize=False))[4]
    want = _noise_replay(sh._hgcfg.seed, 17, 6, 192, 0.02).reshape(12, 16)
    inner = (raw > 0.05) & (raw < 2.95)
    assert inner.mean() > 0.2 and _noise_error_ok(noisy, raw, want, inner)
    assert torch.equal(sh.depth_frame(0)[4], sh.render_depth()[4])


def test_refusals(world):
    from humanoid import _native as N
    env = world["env"]
    out = torch.full((env.num_envs, 12, 16), SENTINEL, device=env.device)
    ok = dict(W=16, H=12)
    cases = [
        ("null sim", dict(sim=None)), ("null cam", dict(cam=None)), ("null out", dict(out=None)),
        ("W = 0", dict(W=0)), ("H < 0", dict(H=-3)), ("too many pixels", dict(W=1024, H=257, stride=1024 * 257)),
        ("stride", dict(stride=191)), ("far <= near", dict(near=1.0, far=1.0)), ("near < 0", dict(near=-0.1)),
        ("fov 0", dict(fov=0.0)), ("fov 180", dict(fov=180.0)), ("noise < 0", dict(noise=-0.01)),
    ]
    for label, kw in cases:
        a = dict(ok, near=0.0, far=3.0, fov=87.0, noise=0.0, stride=192, sim="env", cam="build", out=out)
        a.update(kw)
        cam = _cam(a["W"], a["H"], a["fov"], a["near"], a["far"], 0, a["noise"]) if a["cam"] == "build" else None
        rc = _raw_call(env, cam, a["out"], a["stride"], sim=a["sim"])
        assert rc == 1, f"{label}: returned {rc}"   # HG_ERR_ARG
        if a["sim"] is not None:
            assert N.lib().hg_last_error(env.sim).startswith(b"hg_render_depth"), label
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert _raw_call(env, _cam(16, 12), out, 192) == 0   # and the accepted call writes every pixel
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


def test_graph_capture(world):
    env = world["env"]
    roots, pitch = DR.scene_set(world["origins"])
    _plant(env, roots, pitch)
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
