"""Measured terrain heights in the privileged frame (terrain.critic_heights, BUILD-DEFINED), CPU
side: the option reaches hg_cfg, and the expectation the GPU cases compare against is pinned to the
reference's own heights.

`expected_height_columns` restates include/hgsim.h's column rule in float32, every operation
rounded on its own, on top of oracle/pipeline_ref.heights (pinned to the reference's _get_heights
by tests/test_oracle_pipeline.py).  tests/test_gpu_critic_heights.py imports it."""
import ctypes
import types

import numpy as np

import pipeline_ref as PR

f32 = np.float32


def expected_height_columns(cfg, root_states, points_xy, hf):
    """[N, P] float32: clip(clip((z - 0.5) - h, -1, 1) * scale, +- clip_observations) with
    h = pipeline_ref.heights (zeros when hf is None: the plane), scale = cfg.c.critic_height_scale.
    cfg: pipeline_ref.Cfg (or any object whose .c carries the hg_cfg fields)."""
    c = cfg.c
    root = np.asarray(root_states, f32)
    pts = np.asarray(points_xy, f32)
    h = np.zeros((root.shape[0], pts.shape[0]), f32) if hf is None else PR.heights(cfg, root, pts, hf).astype(f32)
    d = ((root[:, 2:3] - f32(0.5)).astype(f32) - h).astype(f32)
    col = (np.clip(d, f32(-1.0), f32(1.0)).astype(f32) * f32(c.critic_height_scale)).astype(f32)
    clip = f32(c.clip_observations)
    return np.clip(col, -clip, clip).astype(f32)


def _cfg_and_model():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    _, js = N.load_model()
    return XBotLCfg(), js


def test_build_hg_cfg_carries_the_height_fields():
    from humanoid import _native as N
    from humanoid.envs.custom.humanoid_env import build_hg_cfg, critic_height_grid
    cfg, js = _cfg_and_model()
    assert cfg.terrain.critic_heights is False
    hc, aux = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.critic_heights == 0 and not hc.critic_height_points and aux["height_grid"] is None
    assert critic_height_grid(cfg) is None
    cfg.terrain.critic_heights = True
    xs, ys = cfg.terrain.measured_points_x, cfg.terrain.measured_points_y
    hc, aux = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js, height_points=0x1000)
    assert hc.critic_heights == len(xs) * len(ys) == 187
    assert hc.critic_height_scale == f32(cfg.normalization.obs_scales.height_measurements) == 5.0
    assert hc.critic_height_points == 0x1000
    # x-major, as _init_height_points (humanoid_env.py:314-328): point k = (x[k // len(y)], y[k % len(y)])
    grid = aux["height_grid"]
    assert grid.dtype == f32 and grid.shape == (187, 2)
    for k in (0, 1, 10, 11, 100, 186):
        assert tuple(grid[k]) == (f32(xs[k // len(ys)]), f32(ys[k % len(ys)]))
    # another grid, another count; the measure_heights flag plays no part
    cfg.terrain.measured_points_x, cfg.terrain.measured_points_y = [-0.3, 0.0, 0.3], [-0.2, 0.0, 0.2]
    cfg.terrain.measure_heights = True
    hc, aux = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.critic_heights == 9 and not hc.critic_height_points
    np.testing.assert_array_equal(aux["height_grid"][:4], np.array([[-0.3, -0.2], [-0.3, 0.0], [-0.3, 0.2], [0.0, -0.2]], f32))
    # the fields sit between the actuator fields and terrain_origins (the command curriculum's two
    # stay the last: tests/test_cmd_curriculum_rule.py)
    F = N.HgCfg
    assert F.act_armature_range.offset < F.critic_heights.offset < F.critic_height_scale.offset
    assert F.critic_height_scale.offset < F.critic_height_points.offset < F.terrain_origins.offset
    assert F.critic_height_points.size == ctypes.sizeof(ctypes.c_void_p)


def test_arena_grows_by_the_height_columns_only():
    """hg_arena_bytes (no GPU needed): the privileged window's rows widen by P floats per frame slot,
    nothing else moves; a bad count sizes nothing."""
    import os
    import pytest
    from humanoid import _native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    L = N.load_library()
    c = N.HgCfg()
    c.num_envs, c.frame_stack, c.c_frame_stack = 64, 15, 3
    base = L.hg_arena_bytes(ctypes.byref(c))
    c.critic_heights = 187
    grown = L.hg_arena_bytes(ctypes.byref(c))
    slots = 3 - 1 + 26  # c_frame_stack - 1 + the window advance
    assert 0 <= grown - base - 64 * slots * 187 * 4 < 256
    for bad in (-1, 1025):
        c.critic_heights = bad
        assert L.hg_arena_bytes(ctypes.byref(c)) == 0


def test_expected_columns_are_the_references_expression(golden):
    """On tests/golden/heights.npz (root states, grid, heightfield and the reference's own
    _get_heights output): the helper equals clip(z - 0.5 - heights, -1, 1) * 5, then the observation
    clip (humanoid_env.py:872-873, :654-657), bit for bit in float32."""
    z = golden("heights.npz")
    ns = types.SimpleNamespace(hf_border=float(z["border_size"]), hf_horizontal_scale=float(z["horizontal_scale"]),
                               hf_vertical_scale=float(z["vertical_scale"]), critic_height_scale=5.0,
                               clip_observations=18.0)
    cfg = types.SimpleNamespace(c=ns)
    root = z["root_states"].astype(f32)
    got = expected_height_columns(cfg, root, z["points_xy"], z["heightfield"])
    gold = z["heights"].astype(f32)
    np.testing.assert_allclose(PR.heights(cfg, root, z["points_xy"], z["heightfield"]), gold, rtol=0, atol=1e-7)
    want = np.clip(np.clip(root[:, 2:3] - f32(0.5) - gold, f32(-1), f32(1)) * f32(5.0), f32(-18), f32(18))
    assert want.dtype == f32 and got.shape == gold.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)  # atol: the pin's own 1e-7 on h, times 5
    assert (got == want).mean() > 0.999
    # the expectation is not degenerate: columns vary, and few sit on a clip bound
    assert (np.ptp(got, axis=1) > 0).mean() > 0.1 and (np.abs(got) == f32(5.0)).mean() < 0.5
    # the plane: clip(z - 0.5, -1, 1) * scale in every column
    flat = expected_height_columns(cfg, root, z["points_xy"], None)
    np.testing.assert_array_equal(flat, np.repeat(np.clip(root[:, 2:3] - f32(0.5), f32(-1), f32(1)) * f32(5.0),
                                                  gold.shape[1], axis=1))
