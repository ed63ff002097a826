"""The depth camera without a GPU: the numpy reference (tests/depth_ref.py) against closed forms,
the fixed scene set against the conditions that keep the GPU comparison honest, the ctypes layout
of hg_depth_cam, and the config plumbing (XBotLCfg.depth -> hg_depth_cam, refusals in Python).

The GPU tests (tests/test_gpu_depth.py) accept a pixel d when lo - SLACK <= d <= hi + SLACK, [lo, hi]
spanning the float64 reference at the pixel centre and its four (+-0.01, +-0.01) pixel corners.
SLACK = 8 x the float32 replay's largest centre-pixel deviation from the float64 centre render
over the scene set: the project allows 4 x for an independent float32 build of the SAME algorithm
(oracle/step_tolerance.py), doubled because the kernel's formulation differs from the reference's.
Measured here (test_scene_set_keeps_the_gpu_test_honest prints it): 5.43e-6 m, held as
REPLAY_DEV = 5.5e-6 m, so SLACK = 4.4e-5 m.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import depth_ref as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REPLAY_DEV = 5.5e-6       # metres: the float32 replay's largest centre deviation (measured 5.43e-6)
SLACK = 8 * REPLAY_DEV    # metres


def _identity_root(x, y, z):
    r = np.zeros(13)
    r[:3] = (x, y, z)
    r[6] = 1.0
    return r


def test_level_camera_over_a_plane():
    cam = DR.camera(16, 12)
    root = _identity_root(1.25, -0.5, 0.8)
    got = DR.render(DR.scene(None), cam, root[None], np.zeros(1))[0, 0]
    fx = cam.W / 2 / np.tan(np.deg2rad(cam.fov) / 2)
    oz = 0.8 + cam.pos[2]
    for r in range(cam.H):
        below = (r + 0.5 - cam.H / 2) / fx          # -d_z
        want = oz / below if below > 0 and oz / below <= cam.far else cam.far
        np.testing.assert_allclose(got[r], want, rtol=1e-12, atol=0)
    assert (got < cam.far).any() and (got == cam.far).any()


def test_sloped_field_and_the_view_from_below():
    """One uniformly sloped field (the two triangles of every cell coplanar): the ray-plane
    intersection; and a camera under a level field looking up (the surface is two-sided)."""
    hs, vs, border = 0.1, 0.005, 4.0
    a, b = 3, -2   # height units per cell in x and y
    i, j = np.meshgrid(np.arange(120), np.arange(120), indexing="ij")
    sc = DR.scene((a * i + b * j).astype(np.int16), hs, vs, border)
    cam = DR.camera(13, 7)
    yaw, pitch = 0.6, np.deg2rad(25.0)
    root = _identity_root(1.7, 2.1, 1.2)
    root[3:7] = DR.quat_from_euler(0.05, -0.08, yaw)
    got = DR.render(sc, cam, root[None], np.array([pitch]))[0, 0]
    o, D = DR.rays(cam, root, pitch, ((0.0, 0.0),), np.float64)
    D = D[0]
    sx, sy = vs * a / hs, vs * b / hs
    plane_o = sx * (o[0] + border) + sy * (o[1] + border)
    t = (plane_o - o[2]) / (D[..., 2] - sx * D[..., 0] - sy * D[..., 1])
    want = np.where((t >= 0) & (t <= cam.far), t, cam.far)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (want < cam.far).mean() > 0.4
    # from below: a level field at 0.2 m, the camera 0.3 m under it, pitched 60 degrees up
    flat = DR.scene(np.full((120, 120), 40, np.int16), hs, vs, border)
    root = _identity_root(1.7, 2.1, -0.1 - cam.pos[2])
    up = np.deg2rad(-60.0)
    got = DR.render(flat, cam, root[None], np.array([up]))[0, 0]
    o, D = DR.rays(cam, root, up, ((0.0, 0.0),), np.float64)
    t = (0.2 - o[2]) / D[0][..., 2]
    want = np.where((t >= 0) & (t <= cam.far), t, cam.far)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert (want < cam.far).all()


def test_scene_set_keeps_the_gpu_test_honest():
    hf, origins, tcfg = DR.terrain_field()
    assert hf.shape == (2100, 2100)
    sc = DR.field_scene(hf, tcfg)
    cam = DR.camera(16, 12)
    roots, pitch = DR.scene_set(origins)
    assert roots.shape == (24, 13) and roots.dtype == np.float32
    lo, hi, ctr = DR.intervals(sc, cam, roots, pitch)
    wide = (hi - lo > 0.05).mean()
    hits = (ctr < cam.far).mean()
    replay = DR.render(sc, cam, roots, pitch, dtype=np.float32)[0].astype(np.float64)
    dev = np.abs(replay - ctr).max()
    excess = np.maximum(np.maximum(lo - replay, replay - hi), 0.0).max()
    other = DR.render(DR.field_scene(hf, tcfg, other_diagonal=True), cam, roots, pitch)[0]
    seen = ((other < lo - 1e-4) | (other > hi + 1e-4)).mean()
    print(f"scene set: wide intervals {wide:.4%}, terrain hits {hits:.1%}, float32 replay centre deviation "
          f"{dev:.3e} m (slack = 8 x), replay excess {excess:.1e}, other diagonal outside {seen:.2%}")
    assert wide <= 0.02            # the interval rule hides next to nothing
    assert hits >= 0.30            # the images show terrain, not sky
    assert excess == 0.0           # the float32 replay of the reference passes its own rule
    assert seen >= 0.01            # the rule sees a wrong tessellation
    assert dev <= REPLAY_DEV       # the slack's source


def test_struct_size_matches_header(tmp_path):
    from humanoid import _native as N
    c = tmp_path / "sz.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hgsim.h"\nint main(){printf("%zu %zu %zu %zu %zu",'
                 'sizeof(hg_depth_cam),offsetof(hg_depth_cam,pos),offsetof(hg_depth_cam,near_clip),'
                 'offsetof(hg_depth_cam,normalize),offsetof(hg_depth_cam,noise));}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    C = N.HgDepthCam
    assert got == [ctypes.sizeof(C), C.pos.offset, C.near_clip.offset, C.normalize.offset, C.noise.offset]
    assert "hg_render_depth" in N.EXPORTS


def test_config_plumbing_and_python_side_refusals():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    d = XBotLCfg.depth
    assert d.use_camera is False and tuple(d.original) == (106, 60) and d.horizontal_fov == 87
    assert list(d.position) == [0.10, 0.0, 0.15] and list(d.angle) == [20, 30]
    assert (d.near_clip, d.far_clip, d.update_interval, d.buffer_len, d.dis_noise, d.normalize) == (0.0, 3.0, 5, 2, 0.0, True)
    cam = N.depth_cam(d)
    assert (cam.width, cam.height, cam.normalize, cam.noise) == (106, 60, 1, 0.0)
    assert cam.horizontal_fov_deg == 87.0 and cam.near_clip == 0.0 and cam.far_clip == 3.0
    assert [cam.pos[k] for k in range(3)] == [np.float32(0.10), 0.0, np.float32(0.15)]
    cam = N.depth_cam(d, normalize=False, noise=0.02, env_stride=2 * 106 * 60)
    assert cam.normalize == 0 and cam.noise == np.float32(0.02)

    def bad(**kw):
        ns = types.SimpleNamespace(**{k: getattr(d, k) for k in dir(d) if not k.startswith("_")})
        stride = kw.pop("env_stride", None)
        for k, v in kw.items():
            setattr(ns, k, v)
        with pytest.raises(ValueError):
            N.depth_cam(ns, env_stride=stride)
    bad(original=(0, 60))
    bad(original=(106, -1))
    bad(original=(1024, 257))          # 263168 > 262144 pixels
    bad(env_stride=106 * 60 - 1)
    bad(far_clip=0.0)                  # far <= near
    bad(near_clip=-0.1)
    bad(horizontal_fov=0.0)
    bad(horizontal_fov=180.0)
    bad(dis_noise=-0.01)
    N.depth_cam(types.SimpleNamespace(**dict({k: getattr(d, k) for k in dir(d) if not k.startswith("_")},
                                             original=(512, 512))))  # 262144 pixels: the largest accepted
