"""Reference for hg_render_depth_robot (include/hgsim.h): the base depth camera with the robot's own
legs in view.  TEST INFRASTRUCTURE ONLY.

Nothing new is computed here; the two independent float64 references are combined:
  - the camera's rays and the terrain's t from tests/depth_ref.py (rays, the analytic plane,
    _rays_field's brute-force Moeller-Trumbore);
  - the shapes' poses and t from tests/view_ref.py (the oracle's forward kinematics, golden-section
    capsules, face-plane boxes), for the rows of its shape table whose body is not body 0;
  - the nearest t wins, a shape winning a tie with the terrain.
Everything runs at the five sub-pixel samples DR.FIVE: lo / hi span them, robot[k] says whether
sample k ended on a shape.  All arithmetic runs in `dtype`, so the same code is the float64
reference and its float32 replay.

Acceptance rule, as in the depth tests: a pixel d passes when lo - slack <= d <= hi + slack, and no
pixel is excluded.
"""
import numpy as np

import depth_ref as DR
import view_ref as VR


def drawn(model):
    """Indices of the shape table's rows that the depth camera draws: every body but body 0."""
    return [k for k, s in enumerate(VR.local_shapes(model)) if s[1] != 0]


def render(sc, cam, model, roots, q, pitch, offsets=DR.FIVE, dtype=np.float64, select=None, rigid=None):
    """(t [K, N, H, W], robot [K, N, H, W] bool) for roots [N, 13], dof_pos q [N, 12] and pitch [N].
    select: the shape-table rows drawn (None: drawn(model)); rigid: body states to pose the shapes
    from instead of forward kinematics."""
    dtype = np.dtype(dtype).type
    sel = drawn(model) if select is None else list(select)
    shapes = VR.world_shapes(model, roots, q, dtype, rigid=rigid)
    far = dtype(cam.far)
    K, N = len(offsets), len(roots)
    T = np.empty((K, N, cam.H, cam.W), dtype)
    R = np.zeros((K, N, cam.H, cam.W), bool)
    for e in range(N):
        o, D = DR.rays(cam, roots[e], pitch[e], offsets, dtype)
        Df = D.reshape(-1, 3)
        if sc.hf is None:
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -o[2] / Df[:, 2]
            tt = np.where(np.isfinite(t) & (t >= 0) & (t <= far), t, far).astype(dtype)
        else:
            tt = np.empty(len(Df), dtype)
            Dp = D.reshape(K, -1, 3)
            for p in range(Dp.shape[1]):  # a pixel's sub-pixel rays together
                tt.reshape(K, -1)[:, p] = DR._rays_field(sc, o, Dp[:, p], far, dtype)
        best, rob = tt.copy(), np.zeros(len(Df), bool)
        for k in sel:
            ts, _ = VR.ray_shape(shapes[e][k], o, Df, far, dtype)
            win = (ts <= far) & (ts <= best)
            best[win], rob[win] = ts[win], True
        T[:, e] = best.reshape(K, cam.H, cam.W)
        R[:, e] = rob.reshape(K, cam.H, cam.W)
    return T, R


def reference(sc, cam, model, roots, q, pitch, select=None, rigid=None):
    """The acceptance data: lo / hi / ctr [N, H, W] float64 and robot [5, N, H, W]."""
    t, rob = render(sc, cam, model, roots, q, pitch, DR.FIVE, np.float64, select, rigid)
    return dict(lo=t.min(0), hi=t.max(0), ctr=t[0], robot=rob)


def failures(ref, d, slack):
    """Pixels of d [N, H, W] outside their interval, as a bool array."""
    d = np.asarray(d, np.float64)
    return ~np.isfinite(d) | (d < ref["lo"] - slack) | (d > ref["hi"] + slack)


# ------------------------------------------------------------------ the fixed scene set
PLANE_PITCH = np.deg2rad(np.array([60.0, 75.0, 45.0])).astype(np.float32)   # planted envs 0, 1, 2
FIELD_PITCH = np.deg2rad(np.array([60.0, 75.0])).astype(np.float32)         # field envs 0, 1
PLANE_SIZES = ((17, 9), (16, 12))   # 17 x 9: 3 x 2 tiles, the last tile column and row one pixel wide
FIELD_SIZE = (17, 9)
HANDS_PITCH = np.float32(np.pi / 2)  # default pose, straight down, 16 x 12: the excluded hands would show


def camera(size):
    """The default base camera (XBotLCfg.depth: position, fov, far_clip) at `size`."""
    return DR.camera(size[0], size[1])


def plane_set(model):
    """(roots [3, 13], dof_pos [3, 12], pitch [3]) of the plane scenes."""
    from test_view_cases import planted
    roots, q = planted(model)
    return roots, q, PLANE_PITCH


def field_set(model):
    """(scene, roots [2, 13], dof_pos [2, 12], pitch [2]) of the heightfield scenes."""
    from test_view_cases import field_scenes
    sc, roots, q, _ = field_scenes(model)
    return sc, roots, q, FIELD_PITCH
