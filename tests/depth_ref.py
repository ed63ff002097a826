"""Reference depth renderer for hg_render_depth (include/hgsim.h).  TEST INFRASTRUCTURE ONLY.

Written to share nothing with the kernel's algorithm (a segment march over the gap function):
every ray is tested, with a two-sided Moeller-Trumbore intersection, against BOTH triangles of
EVERY cell in the xy bounding box of its segment [0, far], and the smallest t >= 0 wins; on a
plane the intersection is analytic.  The camera conventions are the header's: camera frame x
forward / y left / z up, world rotation R_base(q normalised) R_y(pitch) with positive pitch looking
down, origin p + R_base pos, row 0 the top and column 0 the left of the image, pixel direction
(1, -(c + 0.5 - W/2) / fx, -(r + 0.5 - H/2) / fx), and t itself the planar depth.

All arithmetic runs in `dtype`, so the same code is the float64 reference and its float32 replay;
`offsets` are sub-pixel shifts (du, dv) added to (c + 0.5, r + 0.5).
"""
import types

import numpy as np


def scene(hf=None, hs=0.1, vs=0.005, border=25.0, other_diagonal=False):
    """hf: int16 [rows, cols] (row = x) or None for the plane z = 0.  other_diagonal splits every
    cell along (i+1,j)-(i,j+1) instead of K_step's (i,j)-(i+1,j+1): a deliberately wrong surface."""
    return types.SimpleNamespace(hf=None if hf is None else np.asarray(hf), hs=hs, vs=vs, border=border,
                                 other_diagonal=other_diagonal)


def camera(width, height, fov_deg=87.0, pos=(0.10, 0.0, 0.15), far=3.0):
    return types.SimpleNamespace(W=int(width), H=int(height), fov=float(fov_deg), pos=tuple(pos), far=float(far))


def _rot(q, dtype):
    """Rotation matrix of the normalised xyzw quaternion."""
    q = np.asarray(q, dtype)
    x, y, z, w = q / np.sqrt((q * q).sum(dtype=dtype))
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype)


def rays(cam, root, pitch, offsets, dtype):
    """Origin [3] and directions [K, H, W, 3] (t = planar depth) of one env's camera, K = len(offsets)."""
    root = np.asarray(root, dtype)
    Rb = _rot(root[3:7], dtype)
    p = dtype(pitch)
    c, s = np.cos(p), np.sin(p)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype)
    R = (Rb @ Ry).astype(dtype)
    o = (root[:3] + Rb @ np.asarray(cam.pos, dtype)).astype(dtype)
    fx = dtype(dtype(cam.W) / dtype(2) / np.tan(np.deg2rad(dtype(cam.fov)) / dtype(2)))
    cc, rr = np.meshgrid(np.arange(cam.W, dtype=dtype), np.arange(cam.H, dtype=dtype))
    out = np.empty((len(offsets), cam.H, cam.W, 3), dtype)
    for k, (du, dv) in enumerate(offsets):
        d = np.stack([np.ones_like(cc), -(cc + dtype(0.5) + dtype(du) - dtype(cam.W) / dtype(2)) / fx,
                      -(rr + dtype(0.5) + dtype(dv) - dtype(cam.H) / dtype(2)) / fx], axis=-1).astype(dtype)
        out[k] = d @ R.T
    return o, out


def _rays_field(sc, o, D, far, dtype):
    """For directions D [K, 3] from one origin: the smallest t in [0, far] at which o + t D[k] meets a
    triangle of the field, else far.  The K rays share the cells of their common bounding box."""
    hs, vs, border = dtype(sc.hs), dtype(sc.vs), dtype(sc.border)
    rows, cols = sc.hf.shape
    res = np.full(len(D), far, dtype)
    fin = np.isfinite(D).all(axis=1) & np.isfinite(o).all()
    if not fin.any():
        return res
    ends = np.concatenate([o[None, :], o[None, :] + far * D[fin]]).astype(np.float64)
    gx, gy = (ends[:, 0] + float(border)) / float(hs), (ends[:, 1] + float(border)) / float(hs)
    i0, i1 = max(int(np.floor(gx.min())) - 1, 0), min(int(np.floor(gx.max())) + 1, rows - 2)
    j0, j1 = max(int(np.floor(gy.min())) - 1, 0), min(int(np.floor(gy.max())) + 1, cols - 2)
    if i0 > i1 or j0 > j1:
        return res
    ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()

    def vert(a, b):
        return np.stack([a.astype(dtype) * hs - border, b.astype(dtype) * hs - border,
                         vs * sc.hf[a, b].astype(dtype)], axis=-1).astype(dtype)
    v00, v10, v01, v11 = vert(ii, jj), vert(ii + 1, jj), vert(ii, jj + 1), vert(ii + 1, jj + 1)
    if sc.other_diagonal:
        A, B, C = np.concatenate([v00, v11]), np.concatenate([v10, v01]), np.concatenate([v01, v10])
    else:  # K_step's: lower (00, 10, 11), upper (00, 01, 11)
        A, B, C = np.concatenate([v00, v00]), np.concatenate([v10, v01]), np.concatenate([v11, v11])
    e1, e2 = B - A, C - A
    tv = o[None, :] - A
    qv = np.cross(tv, e1)
    tn = (e2 * qv).sum(-1, dtype=dtype)
    eps = dtype(16) * np.finfo(dtype).eps
    for k in np.nonzero(fin)[0]:
        pv = np.cross(D[k][None, :], e2)
        det = (e1 * pv).sum(-1, dtype=dtype)
        ok = det != 0
        inv = dtype(1) / np.where(ok, det, dtype(1))
        u = (tv * pv).sum(-1, dtype=dtype) * inv
        v = (qv * D[k][None, :]).sum(-1, dtype=dtype) * inv
        t = tn * inv
        hit = ok & (u >= -eps) & (v >= -eps) & (u + v <= dtype(1) + eps) & (t >= 0) & (t <= far)
        if hit.any():
            res[k] = t[hit].min()
    return res


def render(sc, cam, roots, pitch, offsets=((0.0, 0.0),), dtype=np.float64):
    """[K, N, H, W] raw planar depth (metres, far where nothing is hit) for roots [N, >= 7] and
    pitch [N] (radians)."""
    dtype = np.dtype(dtype).type
    roots = np.asarray(roots)
    far = dtype(cam.far)
    out = np.empty((len(offsets), len(roots), cam.H, cam.W), dtype)
    for e in range(len(roots)):
        o, D = rays(cam, roots[e], pitch[e], offsets, dtype)
        if sc.hf is None:
            if not (np.all(np.isfinite(o)) and np.all(np.isfinite(D))):
                out[:, e] = far
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -o[2] / D[..., 2]
            out[:, e] = np.where(np.isfinite(t) & (t >= 0) & (t <= far), t, far)
            continue
        for r in range(cam.H):
            for c in range(cam.W):  # a pixel's sub-pixel rays together
                out[:, e, r, c] = _rays_field(sc, o, D[:, r, c], far, dtype)
    return out


EPS_PIX = 0.01
FIVE = ((0.0, 0.0), (-EPS_PIX, -EPS_PIX), (-EPS_PIX, EPS_PIX), (EPS_PIX, -EPS_PIX), (EPS_PIX, EPS_PIX))


def intervals(sc, cam, roots, pitch):
    """The acceptance interval of every pixel: (lo, hi, centre), each [N, H, W] float64 — the minimum
    and maximum of the float64 render at the pixel centre and at its four (+-0.01, +-0.01) pixel
    corners.  A GPU pixel d passes when lo - slack <= d <= hi + slack; no pixel is excluded."""
    r = render(sc, cam, roots, pitch, FIVE, np.float64)
    return r.min(axis=0), r.max(axis=0), r[0]


# ---- the fixed scene set of tests/test_depth_ref.py and tests/test_gpu_depth.py
SCENE_ENVS = 24


def quat_from_euler(roll, pitch, yaw):
    """xyzw, rotation Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = (np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2),
                              np.cos(yaw / 2), np.sin(yaw / 2))
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy], axis=-1)


def scene_set(env_origins, n=SCENE_ENVS):
    """Root states [n, 13] (rounded to float32) and camera pitches [n] (float32, radians) of the scene
    set: env e stands on env_origins[randint(0, 20), e % 20] plus a uniform +-2 m xy offset at origin z
    + 0.95, yaw uniform in +-pi (every fourth env an exact 0, pi/2, pi, -pi/2), roll and pitch uniform
    in +-0.15 rad, camera pitch uniform in [20, 30] degrees; all from RandomState(7)."""
    rs = np.random.RandomState(7)
    roots = np.zeros((n, 13), np.float64)
    exact = [0.0, np.pi / 2, np.pi, -np.pi / 2]
    pitch = np.zeros(n)
    for e in range(n):
        org = env_origins[rs.randint(0, 20), e % 20]
        xy = rs.uniform(-2.0, 2.0, size=2)
        yaw = rs.uniform(-np.pi, np.pi)
        if e % 4 == 3:
            yaw = exact[(e // 4) % 4]
        rp = rs.uniform(-0.15, 0.15, size=2)
        roots[e, :3] = (org[0] + xy[0], org[1] + xy[1], org[2] + 0.95)
        roots[e, 3:7] = quat_from_euler(rp[0], rp[1], yaw)
        pitch[e] = np.deg2rad(rs.uniform(20.0, 30.0))
    return roots.astype(np.float32), pitch.astype(np.float32)


def terrain_field():
    """The scene set's terrain: XBotLCfg's heightfield generated under np.random.seed(5) (what
    _make_env's envs build): (int16 [2100, 2100] height samples, env_origins [20, 20, 3], terrain cfg)."""
    from humanoid.envs import XBotLCfg
    from humanoid.utils.terrain import HumanoidTerrain
    cfg = XBotLCfg()
    cfg.terrain.mesh_type = "heightfield"
    saved = np.random.get_state()
    np.random.seed(5)
    try:
        ter = HumanoidTerrain(cfg.terrain, SCENE_ENVS)
    finally:
        np.random.set_state(saved)
    return np.asarray(ter.heightsamples, np.int16), np.asarray(ter.env_origins, np.float64), cfg.terrain


def field_scene(hf, tcfg, other_diagonal=False):
    """The scene with the float32 scales the device hg_cfg carries."""
    f = np.float32
    return scene(hf, float(f(tcfg.horizontal_scale)), float(f(tcfg.vertical_scale)), float(f(tcfg.border_size)),
                 other_diagonal)


def _level_root(x, y, z, yaw):
    root = np.zeros(13, np.float64)
    root[:3] = (x, y, z)
    root[3:7] = quat_from_euler(0.0, 0.0, yaw)
    return root


def degenerate_set(env_origins):
    """Five level bases (identity roll and pitch): yaw exactly 0, pi/2, pi, -pi/2 with camera pitch 0
    (at an odd image width the centre column then runs parallel to a grid axis), and one with camera
    pitch exactly pi/2 (float32), whose central ray points straight down.  (roots [5, 13] float32,
    pitch [5] float32)."""
    roots, pitch = [], []
    for k, yaw in enumerate((0.0, np.pi / 2, np.pi, -np.pi / 2, 0.3)):
        org = env_origins[6 + 2 * k, 3 + 3 * k]
        roots.append(_level_root(org[0] + 0.37, org[1] - 0.21, org[2] + 0.95, yaw))
        pitch.append(np.pi / 2 if k == 4 else 0.0)
    return np.asarray(roots).astype(np.float32), np.asarray(pitch, np.float32)


def extent_set(sc, env_origins):
    """Four envs at the field's limits: 0.5 m inside the x = -border edge looking outward, 0.5 m
    outside it looking in, 0.3 m under the local surface looking up, and a NaN root position.
    (roots [4, 13] float32, pitch [4] float32)."""
    y = float(env_origins[3, 7, 1]) + 0.13
    xin, xout = -sc.border + 0.5, -sc.border - 0.5
    org = env_origins[12, 9]
    gi, gj = int((org[0] + sc.border) / sc.hs), int((org[1] + sc.border) / sc.hs)
    under = sc.vs * float(sc.hf[gi - 3:gi + 4, gj - 3:gj + 4].min()) - 0.3
    roots = [_level_root(xin, y, 0.95, np.pi), _level_root(xout, y, 0.95, 0.0),
             _level_root(org[0] + 0.02, org[1] + 0.03, under, 0.7), _level_root(np.nan, 1.0, 0.95, 0.0)]
    pitch = [np.deg2rad(45.0), np.deg2rad(25.0), np.deg2rad(-60.0), np.deg2rad(25.0)]
    return np.asarray(roots).astype(np.float32), np.asarray(pitch, np.float32)
