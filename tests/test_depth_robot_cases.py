"""The depth camera's view of the robot's own legs without a GPU: the conditions that keep the GPU
comparison (tests/test_gpu_depth_robot.py) honest, checked on the combined float64 reference of
tests/depth_robot_ref.py alone; the shapes that are NOT drawn; the host-compiled pixel rectangle of
csrc/hg_depth_robot.h against the reference's rays; and the config field.

SLACK is 8 x the largest centre deviation of the reference's own float32 replay on the scene set
(4 x for an independent float32 build, doubled because the kernel's formulation differs from the
reference's).  REPLAY_DEV holds the measured deviation — 3.000e-5 m at the env planted 180 m out,
where the reference's float32 world coordinates carry a 15 um ulp; 1.793e-5 m on the heightfield —
and test_scene_set_keeps_the_gpu_test_honest checks that the measurement stays within [1/2, 1] of it.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import depth_ref as DR
import depth_robot_ref as RR
import view_ref as VR
from test_view_cases import CSRC, REPO, _hipcc

SHIM = os.path.join(REPO, "tests", "depth_robot_host_shim.hip")

REPLAY_DEV = 3.1e-5      # metres (measured 3.000e-5: plane, 16 x 12, the env 180 m out)
SLACK = 8 * REPLAY_DEV

f32 = np.float32


@pytest.fixture(scope="module")
def model():
    from humanoid import _native as N
    return N.load_model()[0]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    so = os.path.join(str(tmp_path_factory.mktemp("depth_robot_host")), "depth_robot_host.so")
    subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-O3", "-std=c++17", "-I", CSRC, SHIM, "-o", so],
                   check=True, capture_output=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.depth_robot_rect_host.restype = None
    L.depth_robot_rect_host.argtypes = [ctypes.c_int, vp, vp, ctypes.c_float, ctypes.c_int, ctypes.c_int, vp]
    return L


def scene_images(model):
    """[(label, scene, camera, roots, dof_pos, pitch)] of the scene set: the three planted poses on the
    plane at 17 x 9 and 16 x 12, the first two field scenes on the heightfield at 17 x 9."""
    roots, q, pitch = RR.plane_set(model)
    out = [(f"plane {w}x{h}", DR.scene(None), RR.camera((w, h)), roots, q, pitch) for w, h in RR.PLANE_SIZES]
    sc, fr, fq, fp = RR.field_set(model)
    out.append(("field %dx%d" % RR.FIELD_SIZE, sc, RR.camera(RR.FIELD_SIZE), fr, fq, fp))
    return out


def test_scene_set_keeps_the_gpu_test_honest(model):
    """Per image: >= 2 % robot and >= 60 % terrain pixels; at most 1 % of the pixels have samples that
    disagree on robot / terrain or an interval wider than 5 cm; the float32 replay passes the rule at
    every pixel and its centre deviation is the slack's source."""
    worst = 0.0
    for label, sc, cam, roots, q, pitch in scene_images(model):
        ref = RR.reference(sc, cam, model, roots, q, pitch)
        t32, _ = RR.render(sc, cam, model, roots, q, pitch, ((0.0, 0.0),), np.float32)
        for e in range(len(roots)):
            rob = ref["robot"][:, e]
            robot = rob.all(0).mean()
            terrain = (~rob.any(0) & (ref["hi"][e] < cam.far)).mean()
            und = ((rob.any(0) != rob.all(0)) | (ref["hi"][e] - ref["lo"][e] > 0.05)).mean()
            dev = np.abs(t32[0, e].astype(np.float64) - ref["ctr"][e]).max()
            worst = max(worst, dev)
            print(f"{label} env {e}: robot {robot:.1%}, terrain {terrain:.1%}, undecided {und:.2%}, nearest t "
                  f"{ref['lo'][e].min():.3f} m, replay deviation {dev:.3e} m")
            assert robot >= 0.02 and terrain >= 0.60, (label, e)
            assert und <= 0.01, (label, e)
        assert not RR.failures(ref, t32[0], SLACK).any(), label
    print(f"scene set: float32 replay centre deviation {worst:.3e} m (held {REPLAY_DEV:.3e}, slack = 8 x)")
    assert 0.5 * REPLAY_DEV <= worst <= REPLAY_DEV


def test_excluded_shapes_are_really_excluded(model):
    """Default pose (planted env 0), camera straight down (pitch 90 degrees), 16 x 12: the hand capsules
    hang 0.35 m under a camera that sees the floor 1.1 m away, so a reference that drew them would
    differ by more than 0.1 m somewhere; one that drew the base box, which contains the camera, would
    be 0 everywhere."""
    roots, q, _ = RR.plane_set(model)
    roots, q, pitch = roots[:1], q[:1], np.array([RR.HANDS_PITCH])
    cam, plane = RR.camera((16, 12)), DR.scene(None)
    loc = VR.local_shapes(model)
    hands = [k for k, s in enumerate(loc) if s[0] == VR.CAPSULE and s[1] == 0]
    box = [k for k, s in enumerate(loc) if s[0] == VR.BASE_BOX]
    assert RR.drawn(model) == [0, 1, 2, 3, 4, 5, 8, 9] and hands == [6, 7] and box == [10]
    real = RR.reference(plane, cam, model, roots, q, pitch)
    with_hands = RR.reference(plane, cam, model, roots, q, pitch, select=RR.drawn(model) + hands)
    diff = np.abs(with_hands["ctr"] - real["ctr"])
    print(f"hands drawn: {(diff > 0.1).sum()} pixels differ by more than 0.1 m (largest {diff.max():.3f} m)")
    assert (diff > 0.1).sum() >= 1
    with_box = RR.reference(plane, cam, model, roots, q, pitch, select=RR.drawn(model) + box)
    assert (with_box["hi"] == 0.0).all()
    assert real["lo"].min() > 0.3


# ---------------------------------------------------------------- the pixel rectangle
FUZZ_SIZE = (13, 7)      # 2 x 1 tiles, the last tile column 5 wide and the tile row 7 high
FUZZ_SHAPES, FUZZ_VIEWS = 60, 40   # 2400 (shape, base pose, pitch) draws


def _fuzz_rows(rs):
    """Camera-relative rows (world axes), float32: capsules and boxes within 1.6 m of the camera
    origin in every direction, so that some straddle the camera plane and some lie behind it; the
    last row non-finite."""
    rows = np.zeros((FUZZ_SHAPES, 16), f32)
    for k in range(FUZZ_SHAPES):
        v = rs.normal(size=3)
        c = v / np.linalg.norm(v) * rs.uniform(0.05, 1.6)
        if k % 2 == 0:
            h = rs.normal(size=3)
            h = h / np.linalg.norm(h) * rs.uniform(0.0, 0.25)
            rows[k, 0], rows[k, 1:4], rows[k, 4:7], rows[k, 7] = 0, c - h, c + h, rs.uniform(0.02, 0.1)
        else:
            rows[k, 0], rows[k, 1:4], rows[k, 4:7] = 1, c, rs.uniform(0.02, 0.15, size=3)
            rows[k, 7:11] = DR.quat_from_euler(*rs.uniform(-np.pi, np.pi, size=3))
    rows[-1, 2] = np.nan
    return rows


def test_rectangle_holds_every_hit_pixel(host):
    """No pixel whose float64 reference ray hits the shape at any of the five samples lies outside the
    shape's rectangle (hd_pixel_rect, compiled for the host)."""
    rs = np.random.RandomState(17)
    W, H = FUZZ_SIZE
    cam = DR.camera(W, H, pos=(0.0, 0.0, 0.0))
    fx = f32(W / 2 / np.tan(np.deg2rad(cam.fov) / 2))
    rows = _fuzz_rows(rs)
    # the views: base rotation and camera pitch; their rays leave the origin
    quats = DR.quat_from_euler(rs.uniform(-0.5, 0.5, FUZZ_VIEWS), rs.uniform(-0.5, 0.5, FUZZ_VIEWS),
                               rs.uniform(-np.pi, np.pi, FUZZ_VIEWS)).astype(f32)
    pitch = np.deg2rad(rs.uniform(-30.0, 90.0, FUZZ_VIEWS)).astype(f32)
    D = np.empty((FUZZ_VIEWS, 5, H, W, 3))
    axes = np.empty((FUZZ_VIEWS, 3, 3), f32)
    for v in range(FUZZ_VIEWS):
        root = np.zeros(13)
        root[3:7] = quats[v]
        o, D[v] = DR.rays(cam, root, pitch[v], DR.FIVE, np.float64)
        assert not o.any()
        Rb = DR._rot(quats[v].astype(np.float64), np.float64)
        c, s = np.cos(np.float64(pitch[v])), np.sin(np.float64(pitch[v]))
        axes[v] = (Rb @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])).T   # rows: fwd, left, up
    rect = np.zeros((FUZZ_SHAPES, FUZZ_VIEWS, 4), f32)
    for k in range(FUZZ_SHAPES):
        rk = np.ascontiguousarray(np.tile(rows[k], (FUZZ_VIEWS, 1)))
        host.depth_robot_rect_host(FUZZ_VIEWS, rk.ctypes.data, axes.ctypes.data, fx, W, H, rect[k].ctypes.data)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    whole = np.array([0, H - 1, 0, W - 1], f32)
    seen = dict(straddle=0, behind=0, border=0, nonfinite=0, empty=0, hit=0)
    ratios, escaped = [], []
    for k in range(FUZZ_SHAPES):
        row = rows[k].astype(np.float64)
        if row[0] == 0:
            t, _ = VR.ray_capsule(np.zeros(3), D.reshape(-1, 3), row[1:4], row[4:7], row[7], cam.far)
            ctr, rho = (row[1:4] + row[4:7]) / 2, np.linalg.norm(row[4:7] - row[1:4]) / 2 + row[7]
        else:
            t, _ = VR.ray_box(np.zeros(3), D.reshape(-1, 3), row[1:4], row[4:7], DR._rot(row[7:11], np.float64), cam.far)
            ctr, rho = row[1:4], np.linalg.norm(row[4:7])
        hit = (t.reshape(FUZZ_VIEWS, 5, H, W) <= cam.far).any(1)
        for v in range(FUZZ_VIEWS):
            r0, r1, c0, c1 = rect[k, v]
            inside = (rr >= r0) & (rr <= r1) & (cc >= c0) & (cc <= c1)
            if (hit[v] & ~inside).any():
                escaped.append((k, v, rect[k, v].tolist(), np.argwhere(hit[v] & ~inside)[0].tolist()))
            if not np.isfinite(row).all():
                seen["nonfinite"] += 1
                assert np.array_equal(rect[k, v], whole) and not hit[v].any()
                continue
            x = float(axes[v, 0].astype(np.float64) @ ctr)
            if x + rho < -1e-3:
                seen["behind"] += 1
                assert not inside.any() and not hit[v].any(), (k, v)
            elif abs(x) < rho - 1e-3:
                seen["straddle"] += 1
                assert np.array_equal(rect[k, v], whole), (k, v)
            elif inside.any() and not inside.all() and (r0 == 0 or c0 == 0 or r1 == H - 1 or c1 == W - 1):
                seen["border"] += 1
            seen["empty"] += int(not inside.any())
            if hit[v].any():
                seen["hit"] += 1
                ratios.append(inside.sum() / hit[v].sum())
    print(f"{FUZZ_SHAPES * FUZZ_VIEWS} draws at {W} x {H}: {seen}; mean rectangle area / hit area "
          f"{np.mean(ratios):.2f} over the {len(ratios)} draws with a hit")
    assert not escaped, escaped[:5]
    assert min(seen.values()) > 0, seen
    assert seen["hit"] >= 200 and seen["border"] >= 50


def test_config_field():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    assert XBotLCfg.depth.draw_robot is False
    assert N.depth_draw_robot(XBotLCfg.depth) is False
    assert N.depth_draw_robot(types.SimpleNamespace(use_camera=True, draw_robot=True)) is True
    assert N.depth_draw_robot(types.SimpleNamespace(use_camera=True)) is False
    with pytest.raises(ValueError):
        N.depth_draw_robot(types.SimpleNamespace(use_camera=False, draw_robot=True))
    assert "hg_render_depth_robot" in N.EXPORTS
