"""The depth camera on planted rays (tests/depth_cases.py) on the GPU: hg_render_depth with a 1 x 1
camera at pos = 0, one env per row, on the table's own field, against the float64 reference at the
same float32 pose and within the bounds tests/test_depth_cases.py measures; then a 17 x 9 image (no
tile multiple) under both pixel-to-lane mappings.
"""
import numpy as np
import pytest
import torch

import depth_cases as DC
import depth_ref as DR
from test_depth_cases import BOUND_LONG, BOUND_ORD, bound
from test_gpu_depth import SENTINEL, _assert_inside, _g, _plant, _raw_call
from test_gpu_parity import _make_env, _need_gpu

pytestmark = pytest.mark.gpu

f32 = np.float32
POSED = [r for r in DC.ROWS if r.ray is None]           # direct rays run on the host march only
FIELD_ROWS = [r for r in POSED if r.kind == "field"]
PLANE_ROWS = [r for r in POSED if r.kind == "plane"]


def _cam(W, H, fov, pos, far):
    from humanoid import _native as N
    c = N.HgDepthCam()
    c.width, c.height, c.horizontal_fov_deg = W, H, fov
    c.pos[0], c.pos[1], c.pos[2] = pos
    c.near_clip, c.far_clip, c.normalize, c.noise = 0.0, far, 0, 0.0
    return c


def _render(env, cam):
    out = torch.full((env.num_envs, cam.height, cam.width), SENTINEL, device=env.device)
    assert _raw_call(env, cam, out, cam.height * cam.width) == 0
    return _g(out)


@pytest.fixture(scope="module")
def field_env():
    """A heightfield env of the table's shape and scales, one env per posed field row, whose height
    samples (the memory hg_cfg.heightfield points to) are overwritten in place with the table's field."""
    _need_gpu()
    env = _make_env(len(FIELD_ROWS), terrain__mesh_type="heightfield", terrain__horizontal_scale=DC.HS,
                    terrain__vertical_scale=DC.VS, terrain__border_size=DC.BORDER, terrain__terrain_length=2.0,
                    terrain__terrain_width=2.0, terrain__num_rows=60, terrain__num_cols=4, terrain__selected=True,
                    terrain__terrain_kwargs={"type": "sloped_terrain", "terrain_kwargs": {"slope": 0.0}},
                    depth__use_camera=True, depth__original=(16, 12))
    hf = DC.field()
    assert tuple(env.height_samples.shape) == hf.shape and env.height_samples.dtype == torch.int16
    c = env._hgcfg
    assert c.heightfield == env.height_samples.data_ptr()
    assert (c.hf_rows, c.hf_cols, c.hf_horizontal_scale, c.hf_vertical_scale, c.hf_border) == (
        DC.NROWS, DC.NCOLS, DC.HS, DC.VS, DC.BORDER)
    env.height_samples.copy_(torch.from_numpy(hf).to(env.device))
    torch.cuda.synchronize()
    return env


def _run_rows(env, rows, sc):
    """Every row's GPU depth (its env's single pixel, rendered at the row's far) and its reference."""
    poses = [DC.pose(r) for r in rows]
    _plant(env, np.stack([p[0] for p in poses]), np.asarray([p[1] for p in poses], f32))
    got = np.empty(len(rows), f32)
    for far in sorted({r.far for r in rows}):
        d = _render(env, _cam(1, 1, DC.FOV, (0.0, 0.0, 0.0), far))
        assert d.shape == (env.num_envs, 1, 1)
        for k, r in enumerate(rows):
            if r.far == far:
                got[k] = d[k, 0, 0]
    ref = np.asarray([DC.reference(r, sc) for r in rows])
    return got, ref


def _check_rows(rows, got, ref):
    bad = []
    for k, r in enumerate(rows):
        err = abs(float(got[k]) - ref[k])
        print(f"{r.name:44s} ref {ref[k]:.9g} gpu {got[k]:.9g} err {err:.2e}")
        ok = np.isfinite(got[k]) and ((got[k] == f32(r.far)) if "guard" in r.tags else err <= bound(r))
        if not ok:
            bad.append((r.name, float(got[k]), float(ref[k])))
    err = np.abs(got.astype(np.float64) - ref)
    long = np.asarray(["long" in r.tags for r in rows])
    print(f"largest deviation: ordinary rows {err[~long].max():.3e} m (bound {BOUND_ORD:.1e})"
          + (f", long rows {err[long].max():.3e} m (bound {BOUND_LONG:.1e})" if long.any() else ""))
    assert not bad, f"{len(bad)} rows outside their bound (name, gpu, reference): {bad}"


def test_field_rows(field_env):
    assert len(FIELD_ROWS) >= 50 and field_env.num_envs == len(FIELD_ROWS)
    got, ref = _run_rows(field_env, FIELD_ROWS, DC.scene())
    _check_rows(FIELD_ROWS, got, ref)


def test_plane_rows():
    _need_gpu()
    env = _make_env(len(PLANE_ROWS), depth__use_camera=True, depth__original=(16, 12))
    assert env._hgcfg.terrain_type == 0 and len(PLANE_ROWS) >= 6
    got, ref = _run_rows(env, PLANE_ROWS, None)
    _check_rows(PLANE_ROWS, got, ref)


IMAGE_POSES = ["tri_lower_oblique", "hit_from_above", "origin_on_vertex_oblique", "outside_in_low_x",
               "edge_origin_high_u_inward", "dgy_zero_pitched"]


def test_image_17x9_both_mappings(field_env, monkeypatch):
    """17 x 9: 3 x 2 tiles, the last column of tiles one pixel wide, the last row one pixel high, the
    second block half empty.  The tile mapping and HG_DEPTH_MAP=rows (read at every call) give the same
    bits, a repeated frame too, and both lie in the reference's intervals."""
    env = field_env
    rows = [next(r for r in DC.ROWS if r.name == n) for n in IMAGE_POSES]
    poses = [DC.pose(r) for r in rows]
    roots, pitch = np.stack([p[0] for p in poses]), np.asarray([p[1] for p in poses], f32)
    _plant(env, roots, pitch)
    pos, far = (0.10, 0.0, 0.15), 3.0
    cam = _cam(17, 9, 87.0, pos, far)
    monkeypatch.delenv("HG_DEPTH_MAP", raising=False)
    tile = _render(env, cam)
    again = _render(env, cam)
    monkeypatch.setenv("HG_DEPTH_MAP", "rows")
    by_rows = _render(env, cam)
    monkeypatch.delenv("HG_DEPTH_MAP")
    n = len(rows)
    assert tile.shape == (env.num_envs, 9, 17) and not (tile == SENTINEL).any()
    assert np.array_equal(tile.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(tile.view(np.uint32), by_rows.view(np.uint32))
    lo, hi, ctr = DR.intervals(DC.scene(), DR.camera(17, 9, 87.0, pos, far), roots, pitch)
    assert (ctr < far).mean() > 0.3
    _assert_inside(tile[:n], lo, hi, "17 x 9, tiles")
    _assert_inside(by_rows[:n], lo, hi, "17 x 9, rows")
