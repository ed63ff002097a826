"""Reference renderer for hg_render_view / hg_view_shapes (include/hgsim.h).  TEST INFRASTRUCTURE ONLY.

Written to share nothing with the kernel's formulation (csrc/hg_view_shapes.h):
  - poses come from the oracle's forward kinematics (oracle/physics_ref.rigid_states), the shape
    table is restated here from the hg_model the tests load;
  - ray / capsule: g(t) = dist(o + t d, segment) - r is convex in t; its minimiser is found by a
    golden-section search over [0, far] and the entry root by bisection on [0, t*] (no quadratic);
  - ray / box: the six face planes, each hit clipped to its face's rectangle (no slabs), in the box
    frame reached through the rotation MATRIX of the quaternion;
  - terrain: depth_ref._rays_field (brute-force two-sided Moeller-Trumbore) or the analytic plane.
Conventions restated from the headers: camera frame x forward / y left / z up with up = world +z,
forward = normalize(target - eye), follow mode adds the base position to eye and target; pixel
(r, c) has the direction fwd - (c + 0.5 - W/2)/fx left - (r + 0.5 - H/2)/fx up and t is the planar
depth; ids 0 sky, 1 terrain, 2 + k shape k; a shape wins a tie with the terrain, the lower index a
tie among shapes; an origin inside a shape is t = 0 with normal -d/|d|; a terrain t equal to far is sky.

All arithmetic runs in `dtype`, so the same code is the float64 reference and its float32 replay.
"""
import types

import numpy as np

import depth_ref as DR

# ---- constants restated from csrc/hg_view_shapes.h
LIGHT = np.array([0.3, 0.2, 0.9]) / np.sqrt(0.3 ** 2 + 0.2 ** 2 + 0.9 ** 2)
AMBIENT, DIFFUSE = 0.35, 0.65
CHECKER = ((0.55, 0.55, 0.50), (0.40, 0.40, 0.36))  # floor(x) + floor(y) even / odd
ALBEDO = {0: (0.85, 0.45, 0.15), 1: (0.20, 0.20, 0.20), 2: (0.25, 0.35, 0.70)}  # by shape kind
SKY = (0.53, 0.71, 0.92)
SKY_U8 = tuple(int(np.rint(255 * v)) for v in SKY)
CAPSULE, FOOT_BOX, BASE_BOX = 0, 1, 2
FIVE = DR.FIVE


def camera(width, height, fov_deg, eye, target, far, mode=0):
    return types.SimpleNamespace(W=int(width), H=int(height), fov=float(fov_deg), eye=tuple(float(v) for v in eye),
                                 target=tuple(float(v) for v in target), far=float(far), mode=int(mode))


def native_cam(cam):
    """The hg_view_cam of a reference camera."""
    from humanoid import _native as N
    return N.view_cam((cam.W, cam.H), cam.fov, cam.eye, cam.target, cam.far, mode=cam.mode)


# ------------------------------------------------------------------ shapes
def local_shapes(model):
    """The body-frame shape table restated from an HgModel: [(kind, body, a, b, r)] — capsule a = p0,
    b = p1; box a = centre, b = half extents."""
    out = []
    for k in range(model.num_capsules):
        if model.capsule_kind[k] == 0:
            out.append((CAPSULE, int(model.capsule_body[k]), np.array(model.capsule_p0[k][:], np.float64),
                        np.array(model.capsule_p1[k][:], np.float64), float(model.capsule_radius[k])))
    nf = model.num_foot_contacts
    pts = np.array([model.contact_pos[c][:] for c in range(model.num_contacts)], np.float64)
    body = np.array([model.contact_body[c] for c in range(model.num_contacts)])
    rad = np.array([model.contact_radius[c] for c in range(model.num_contacts)])
    seen = []
    for c in range(nf):
        if body[c] not in seen:
            seen.append(int(body[c]))
    for b in seen:
        p = np.concatenate([pts[:nf][body[:nf] == b], np.zeros((1, 3))])
        out.append((FOOT_BOX, b, (p.min(0) + p.max(0)) / 2, (p.max(0) - p.min(0)) / 2, 0.0))
    sel = (body == 0) & (rad == 0) & (np.arange(len(body)) >= nf)
    if sel.any():
        p = pts[sel]
        out.append((BASE_BOX, 0, (p.min(0) + p.max(0)) / 2, (p.max(0) - p.min(0)) / 2, 0.0))
    return out[:16]


def _rot(q, dtype):
    return DR._rot(q, dtype)


def world_shapes(model, roots, dof_pos, dtype=np.float64, rigid=None):
    """Per env a list of world shapes: ("capsule", kind, p0, p1, r) / ("box", kind, centre, half, R, quat).
    Poses: the oracle's FK of (roots, dof_pos), or the given rigid [n, 13, 13] body states."""
    import physics_ref as PR
    dtype = np.dtype(dtype).type
    roots = np.atleast_2d(np.asarray(roots))
    if rigid is None:
        rigid = PR.rigid_states(model, roots[:, :13], dof_pos, np.zeros_like(np.asarray(dof_pos, np.float64)),
                                precision="f64" if dtype is np.float64 else "f32")
    rigid = np.asarray(rigid).astype(dtype)
    loc = local_shapes(model)
    out = []
    for e in range(len(roots)):
        row = []
        for kind, b, a, bb, r in loc:
            R = _rot(rigid[e, b, 3:7], dtype)
            pos = rigid[e, b, :3]
            wa = (pos + R @ a.astype(dtype)).astype(dtype)
            if kind == CAPSULE:
                row.append(("capsule", kind, wa, (pos + R @ bb.astype(dtype)).astype(dtype), dtype(r)))
            else:
                row.append(("box", kind, wa, bb.astype(dtype), R, rigid[e, b, 3:7]))
        out.append(row)
    return out


def table_array(shapes):
    """[n, ns, 16] float64 table in hg_view_shapes' row layout."""
    out = np.zeros((len(shapes), len(shapes[0]), 16))
    for e, row in enumerate(shapes):
        for k, s in enumerate(row):
            out[e, k, 0] = s[1]
            out[e, k, 1:4] = s[2]
            out[e, k, 4:7] = s[3]
            if s[0] == "capsule":
                out[e, k, 7] = s[4]
            else:
                out[e, k, 7:11] = s[5]
    return out


# ------------------------------------------------------------------ rays
def rays(cam, base, offsets, dtype):
    """Origin [3] and directions [K, H, W, 3] of the camera for an env whose base position is `base`."""
    dtype = np.dtype(dtype).type
    eye, tgt = np.asarray(cam.eye, np.float32).astype(dtype), np.asarray(cam.target, np.float32).astype(dtype)
    f = tgt - eye
    f = f / np.sqrt((f * f).sum(dtype=dtype))
    left = np.cross(np.array([0, 0, 1], dtype), f)
    left = left / np.sqrt((left * left).sum(dtype=dtype))
    up = np.cross(f, left)
    o = eye + (np.asarray(base, dtype)[:3] if cam.mode == 1 else dtype(0))
    fx = dtype(dtype(cam.W) / dtype(2) / np.tan(np.deg2rad(dtype(cam.fov)) / dtype(2)))
    cc, rr = np.meshgrid(np.arange(cam.W, dtype=dtype), np.arange(cam.H, dtype=dtype))
    D = np.empty((len(offsets), cam.H, cam.W, 3), dtype)
    for k, (du, dv) in enumerate(offsets):
        y = -(cc + dtype(0.5) + dtype(du) - dtype(cam.W) / dtype(2)) / fx
        z = -(rr + dtype(0.5) + dtype(dv) - dtype(cam.H) / dtype(2)) / fx
        D[k] = f + y[..., None] * left + z[..., None] * up
    return o.astype(dtype), D


GOLD = (np.sqrt(5.0) - 1.0) / 2.0


def ray_capsule(o, D, p0, p1, r, far, dtype=np.float64):
    """First t in [0, far] of rays o [3] + t D [n, 3] on the capsule, inf on a miss, and the unit
    outward normal [n, 3] (-d/|d| at t = 0)."""
    dtype = np.dtype(dtype).type
    o, D, p0, p1 = (np.asarray(v, dtype) for v in (o, D, p0, p1))
    n = len(D)
    t_out = np.full(n, np.inf, dtype)
    nrm = np.zeros((n, 3), dtype)
    fin = np.isfinite(D).all(1) & bool(np.isfinite(o).all() and np.isfinite(p0).all() and np.isfinite(p1).all()
                                       and np.isfinite(r) and np.isfinite(far))
    ba = p1 - p0
    L2 = (ba * ba).sum(dtype=dtype)

    def closest(t):  # the segment's point nearest o + t D
        x = o[None, :] + t[:, None] * D - p0[None, :]
        s = np.clip((x @ ba) / L2, 0, 1) if L2 > 0 else np.zeros(n, dtype)
        return x - s[:, None] * ba[None, :]

    def g(t):
        w = closest(t)
        return np.sqrt((w * w).sum(1, dtype=dtype)) - dtype(r)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.zeros(n, dtype), np.full(n, far, dtype)
        x1, x2 = hi - dtype(GOLD) * (hi - lo), lo + dtype(GOLD) * (hi - lo)
        g1, g2 = g(x1), g(x2)
        for _ in range(90):
            left = g1 < g2
            hi, lo = np.where(left, x2, hi), np.where(left, lo, x1)
            nx1, nx2 = hi - dtype(GOLD) * (hi - lo), lo + dtype(GOLD) * (hi - lo)
            x1, x2 = nx1, nx2
            g1, g2 = g(x1), g(x2)
        # candidates for a point at or below zero: the bracket's probes and the interval's ends
        cand = np.stack([x1, x2, lo, hi, np.zeros(n, dtype), np.full(n, far, dtype)])
        gv = np.stack([g(c) for c in cand])
        neg = gv <= 0
        tm = np.where(neg, cand, np.inf).min(0)        # the earliest candidate inside
        g0 = g(np.zeros(n, dtype))
        inside = fin & (g0 <= 0)
        hit = fin & ~inside & np.isfinite(tm)
        a, b = np.zeros(n, dtype), np.where(hit, tm, dtype(0))
        for _ in range(70):
            m = (a + b) / dtype(2)
            below = g(m) <= 0
            b, a = np.where(below, m, b), np.where(below, a, m)
        t_out[hit] = b[hit]
        t_out[inside] = 0
        w = closest(np.where(hit, b, dtype(0)))
        wn = np.sqrt((w * w).sum(1, dtype=dtype))
        nrm[hit] = (w / np.where(wn > 0, wn, 1)[:, None])[hit]
        dn = np.sqrt((D * D).sum(1, dtype=dtype))
        nrm[inside] = (-D / dn[:, None])[inside]
    return t_out, nrm


def ray_box(o, D, c, h, R, far, dtype=np.float64):
    """As ray_capsule, for the box of centre c, half extents h and rotation matrix R."""
    dtype = np.dtype(dtype).type
    o, D, c, h, R = (np.asarray(v, dtype) for v in (o, D, c, h, R))
    n = len(D)
    t_out = np.full(n, np.inf, dtype)
    nrm = np.zeros((n, 3), dtype)
    fin = np.isfinite(D).all(1) & bool(np.isfinite(o).all() and np.isfinite(c).all() and np.isfinite(h).all()
                                       and np.isfinite(R).all() and np.isfinite(far))
    with np.errstate(invalid="ignore"):
        ol = R.T @ (o - c)
    dl = D @ R            # rows: R^T d
    inside = fin & bool((np.abs(ol) <= h).all())
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for ax in range(3):
            oth = [i for i in range(3) if i != ax]
            for sg in (-1.0, 1.0):
                t = (dtype(sg) * h[ax] - ol[ax]) / dl[:, ax]
                p = ol[None, :] + t[:, None] * dl
                ok = fin & np.isfinite(t) & (t >= 0) & (t <= far) & (np.abs(p[:, oth[0]]) <= h[oth[0]]) & \
                    (np.abs(p[:, oth[1]]) <= h[oth[1]]) & (t < t_out)
                t_out[ok] = t[ok]
                nl = np.zeros(3, dtype)
                nl[ax] = sg
                nrm[ok] = R @ nl
    t_out[inside] = 0
    dn = np.sqrt((D * D).sum(1, dtype=dtype))
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm[inside] = (-D / dn[:, None])[inside]
    t_out[~fin] = np.inf
    return t_out, nrm


def ray_shape(s, o, D, far, dtype):
    if s[0] == "capsule":
        return ray_capsule(o, D, s[2], s[3], s[4], far, dtype)
    return ray_box(o, D, s[2], s[3], s[4], far, dtype)


def shade(kind_or_none, hit_xy, n, d):
    """float64 colour in [0, 255] (before rounding) [.., 3]: kind_or_none None = terrain (checker at
    hit_xy), else the shape kind."""
    n, d = np.asarray(n, np.float64), np.asarray(d, np.float64)
    flip = (n * d).sum(-1) > 0
    n = np.where(flip[..., None], -n, n)
    k = AMBIENT + DIFFUSE * np.maximum(0.0, n @ LIGHT)
    if kind_or_none is None:
        par = (np.floor(hit_xy[..., 0]) + np.floor(hit_xy[..., 1])).astype(np.int64) & 1
        al = np.where(par[..., None] == 0, np.array(CHECKER[0]), np.array(CHECKER[1]))
    else:
        al = np.array(ALBEDO[kind_or_none])
    return 255.0 * np.clip(al * k[..., None], 0.0, 1.0)


def _terrain_key(sc, x, y):
    """(checker square, triangle) of world points: int64 [..., 5] (floor x, floor y, i, j, lower), and
    the triangle's unit normal."""
    fx, fy = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    if sc.hf is None:
        z = np.zeros_like(fx)
        nrm = np.zeros(x.shape + (3,))
        nrm[..., 2] = 1.0
        return np.stack([fx, fy, z, z, z], -1), nrm
    rows, cols = sc.hf.shape
    gx, gy = (x + sc.border) / sc.hs, (y + sc.border) / sc.hs
    i = np.clip(np.floor(gx).astype(np.int64), 0, rows - 2)
    j = np.clip(np.floor(gy).astype(np.int64), 0, cols - 2)
    lower = (gx - i) >= (gy - j)
    H = sc.hf.astype(np.float64) * sc.vs
    h00, h10, h01, h11 = H[i, j], H[i + 1, j], H[i, j + 1], H[i + 1, j + 1]
    dx = np.where(lower, h10 - h00, h11 - h01) / sc.hs
    dy = np.where(lower, h11 - h10, h01 - h00) / sc.hs
    inv = 1 / np.sqrt(dx * dx + dy * dy + 1)
    return np.stack([fx, fy, i, j, lower.astype(np.int64)], -1), np.stack([-dx * inv, -dy * inv, inv], -1)


def render(sc, cam, shapes, bases, offsets=((0.0, 0.0),), dtype=np.float64):
    """Render envs (shapes[e] from world_shapes, bases[e] the base position) -> dict of
    t [K, N, H, W] (far where nothing is hit), ids [K, N, H, W] int, key [K, N, H, W, 5] (terrain
    pixels' checker square and triangle, else 0) and rgb [N, H, W, 3] float64, the unrounded colour
    of sample 0."""
    dtype = np.dtype(dtype).type
    K, N = len(offsets), len(shapes)
    far = dtype(cam.far)
    T = np.empty((K, N, cam.H, cam.W), dtype)
    I = np.zeros((K, N, cam.H, cam.W), np.int64)
    KEY = np.zeros((K, N, cam.H, cam.W, 5), np.int64)
    RGB = np.zeros((N, cam.H, cam.W, 3))
    for e in range(N):
        o, D = rays(cam, bases[e], offsets, dtype)
        Df = D.reshape(-1, 3)
        n = len(Df)
        # terrain
        if not np.isfinite(o).all():
            tt = np.full(n, far, dtype)
        elif sc.hf is None:
            with np.errstate(divide="ignore", invalid="ignore"):
                t = -o[2] / Df[:, 2]
            tt = np.where(np.isfinite(t) & (t >= 0) & (t <= far), t, far).astype(dtype)
        else:
            tt = np.empty(n, dtype)
            Dp = D.reshape(K, -1, 3)
            for p in range(Dp.shape[1]):  # a pixel's sub-pixel rays together
                tt.reshape(K, -1)[:, p] = DR._rays_field(sc, o, Dp[:, p], far, dtype)
        ids = np.where(tt < far, 1, 0)
        best = tt.copy()
        nrm = np.zeros((n, 3), dtype)
        kinds = np.full(n, -1)
        for k, s in enumerate(shapes[e]):
            ts, ns = ray_shape(s, o, Df, far, dtype)
            win = (ts <= far) & np.where(ids >= 2, ts < best, ts <= best)
            best[win], ids[win], nrm[win], kinds[win] = ts[win], 2 + k, ns[win], s[1]
        T[:, e] = best.reshape(K, cam.H, cam.W)
        I[:, e] = ids.reshape(K, cam.H, cam.W)
        hit = o.astype(np.float64)[None, :] + best.astype(np.float64)[:, None] * Df.astype(np.float64)
        ter = ids == 1
        key, tn = _terrain_key(sc, np.where(ter, hit[:, 0], 0.0), np.where(ter, hit[:, 1], 0.0))
        key[~ter] = 0
        KEY[:, e] = key.reshape(K, cam.H, cam.W, 5)
        # colour of sample 0
        m = cam.H * cam.W
        col = np.tile(255.0 * np.array(SKY), (m, 1))
        d0 = Df[:m].astype(np.float64)
        t0 = ter[:m]
        if t0.any():
            col[t0] = shade(None, hit[:m][t0], tn[:m][t0], d0[t0])
        for kind in ALBEDO:
            sel = (ids[:m] >= 2) & (kinds[:m] == kind)
            if sel.any():
                col[sel] = shade(kind, None, nrm[:m][sel].astype(np.float64), d0[sel])
        RGB[e] = col.reshape(cam.H, cam.W, 3)
    return dict(t=T, ids=I, key=KEY, rgb=RGB)


def reference(sc, cam, shapes, bases):
    """The acceptance data of an image set: lo / hi [N, H, W] (min / max t over FIVE), idset
    [5, N, H, W], decided [N, H, W] (the five samples agree on the id and, on terrain, on checker
    square and triangle), rgb [N, H, W, 3] float64 at the centre."""
    r = render(sc, cam, shapes, bases, FIVE, np.float64)
    same = (r["ids"] == r["ids"][:1]).all(0) & (r["key"] == r["key"][:1]).all(0).all(-1)
    return dict(lo=r["t"].min(0), hi=r["t"].max(0), ctr=r["t"][0], idset=r["ids"], decided=same, rgb=r["rgb"],
                far=cam.far)


def failures(ref, depth, ids, rgb, slack):
    """Counts of pixels failing the acceptance rule: (depth, id, colour); None inputs are not checked."""
    bad_d = bad_i = bad_c = 0
    if depth is not None:
        d = np.asarray(depth, np.float64)
        bad_d = int((~np.isfinite(d) | (d < ref["lo"] - slack) | (d > ref["hi"] + slack)).sum())
    if ids is not None:
        bad_i = int((~(np.asarray(ids)[None] == ref["idset"]).any(0)).sum())
    if rgb is not None:
        diff = np.abs(np.asarray(rgb, np.float64) - np.rint(ref["rgb"])).max(-1)
        bad_c = int(((diff > 1) & ref["decided"]).sum())
    return bad_d, bad_i, bad_c


# ------------------------------------------------------------------ the fixed scene set
def quat_from_euler(roll, pitch, yaw):
    return DR.quat_from_euler(roll, pitch, yaw)


def planted_states(default_dof_pos, lower, upper, origin=(0.0, 0.0, 0.0)):
    """Three planted envs (float32): root_states [3, 13] and dof_pos [3, 12] —
    env 0 upright in the default pose, env 1 tilted in a deep knee bend, env 2 180 m from the
    origin with every joint at a limit (alternating lower / upper).  `origin` shifts envs 0 and 1."""
    roots = np.zeros((3, 13))
    roots[:, 6] = 1.0
    ox, oy, oz = origin
    roots[0, :3] = (ox + 0.31, oy - 0.23, oz + 0.95)
    roots[0, 3:7] = quat_from_euler(0.0, 0.0, 0.4)
    roots[1, :3] = (ox + 1.47, oy + 1.13, oz + 0.80)
    roots[1, 3:7] = quat_from_euler(0.12, -0.2, -1.1)
    roots[2, :3] = (180.37, -20.21, 0.97)
    roots[2, 3:7] = quat_from_euler(-0.05, 0.08, 2.5)
    q = np.tile(np.asarray(default_dof_pos, np.float64), (3, 1))
    for side in (0, 6):  # hip pitch, knee, ankle pitch of either leg
        q[1, side + 2] += 0.5
        q[1, side + 3] -= 1.0
        q[1, side + 4] += 0.5
    lim = np.where(np.arange(12) % 2 == 0, np.asarray(lower), np.asarray(upper))
    q[2] = lim
    return roots.astype(np.float32), q.astype(np.float32)


def world_cameras(W, H, base, far=12.0, shift=(0.0, 0.0)):
    """Four world cameras on the robot whose base is at `base`: in front, to the side, above looking
    down (not parallel to z), and low, looking up past the robot at the sky."""
    b = np.asarray(base, np.float64)[:3]
    sh = np.array([shift[0], shift[1], 0.0])  # moves every eye: how a scene is kept under the undecided cap
    mk = lambda e, t: camera(W, H, 60.0, b + np.array(e) + sh, b + np.array(t), far, 0)  # noqa: E731
    return {"front": mk((2.6, 0.15, 0.1), (0.0, 0.0, -0.3)), "side": mk((0.2, -2.4, -0.2), (0.0, 0.0, -0.35)),
            "above": mk((0.35, 0.2, 1.9), (0.0, 0.0, -0.5)), "low": mk((1.9, -0.6, -0.7), (0.0, 0.0, 0.1))}


def plane_scenes(roots):
    """[(name, env, camera)] of the plane scene set: envs 0 (default pose) and 1 (knee bend) under the
    four world cameras, image sizes 20 x 12 and 9 x 7 (no tile multiples; the 64 x 36 images are the heightfield's)."""
    out = []
    sizes = {("front", 0): (20, 12), ("side", 0): (20, 12), ("above", 0): (9, 7), ("low", 0): (20, 12),
             ("front", 1): (20, 12), ("side", 1): (20, 12), ("above", 1): (20, 12), ("low", 1): (9, 7)}
    for e in (0, 1):
        for name in ("front", "side", "above", "low"):
            W, H = sizes[(name, e)]
            shift = {("above", 0): (-0.07, -0.07), ("low", 1): (0.07, 0.07), ("side", 1): (0.0, -0.13), ("front", 1): (0.0, -0.13)}.get((name, e), (0.0, 0.0))
            out.append((f"{name}-env{e}-{W}x{H}", e, world_cameras(W, H, roots[e], shift=shift)[name]))
    return out


def follow_camera(W, H, fov=16.0, eye=(0.97, -0.83, 1.62), target=(0.0, 0.0, -0.5), far=3.6):
    """A follow camera (mode 1) for the heightfield scenes: a long lens looking steeply down at legs
    and ground.  On 0.1 m cells a +-0.01 pixel footprint must stay far below a cell for the five
    samples to agree on the triangle (the 2 % undecided cap), which the viewer's 60 degree lens at
    these image sizes does not give; and the reference's brute-force terrain search is quadratic in
    far / horizontal_scale."""
    return camera(W, H, fov, eye, target, far, 1)


def outside_camera(sc, y):
    """A world camera 3 m outside the field's x = -border edge and 3 m under the ground, looking in and
    up through a long lens (see follow_camera) at the border's underside near world y."""
    return camera(20, 12, 8.0, (-sc.border - 3.0, y, -3.0), (-sc.border + 0.5, y + 0.9, 0.5), 8.0, 0)


def decided_camera(sc, shapes, base, W=20, H=12, cap=0.02):
    """The first "front" world camera on `base`, over a fixed list of eye shifts, whose reference image
    keeps its undecided pixels within `cap`: (camera, reference), or None.  For poses only known at
    run time (a reset's draw), where the camera cannot be moved by hand."""
    for dx in (0.0, 0.07, -0.07, 0.13, -0.13):
        for dy in (0.0, -0.13, 0.13, -0.07, 0.07):
            cam = world_cameras(W, H, base, shift=(dx, dy))["front"]
            ref = reference(sc, cam, shapes, [np.asarray(base)[:3]])
            if 1.0 - ref["decided"].mean() <= cap:
                return cam, ref
    return None


def rough_origin(sc, env_origins):
    """The env origin of the suite's heightfield (depth_ref.terrain_field: XBotLCfg's proportions hold
    no stairs) whose 4 m x 4 m neighbourhood has the largest height spread: stepped obstacles, the
    nearest thing to a stair edge the field has."""
    best, arg = -1.0, None
    for i in range(env_origins.shape[0]):
        for j in range(env_origins.shape[1]):
            o = env_origins[i, j]
            gi, gj = int((o[0] + sc.border) / sc.hs), int((o[1] + sc.border) / sc.hs)
            s = float(sc.hf[gi - 20:gi + 20, gj - 20:gj + 20].astype(np.float64).std())
            if s > best:
                best, arg = s, o
    return np.asarray(arg, np.float64)
