"""Planted rays for the depth march (depth_march, csrc/hg_depth.hip).  TEST INFRASTRUCTURE ONLY.

One hand-built int16 field at scales that are exact in binary (hs = 0.25 m, vs = 2^-8 m, border =
4 m; 512 x 64 vertices, x the long axis) and one table, ROWS: one ray per row, each named after the
branch of the march it is planted on.  tests/test_depth_cases.py runs the table through a host build
of the march and tests/test_gpu_depth_cases.py through hg_render_depth (one env per row, a 1 x 1
camera with pos = 0, whose single pixel looks along the camera's x axis), both against the float64
reference of tests/depth_ref.py.

The field (heights in units of vs; X(i) = 0.25 i - 4, Y(j) = 0.25 j - 4):
  level      128 (0.5 m) wherever nothing else is said
  kerb       i in [0, 6], j >= 44: 128 + 16 (j - 44), a ramp in y that reaches the low x edge
  slope      i in [40, 80]: 128 + 8 (i - 40) + 4 j, one plane (both triangles of a cell coplanar)
  saddles    i in [90, 110], j in [16, 48]: 128 + 64 pat[(i - j) % 3], pat = (0, 1, -1).  Cells with
             (i - j) % 3 == 0 have h00 = h11, h10 = -h01 = 0.25 m about h00 (one tilted plane: swapping
             p[1] and p[C] flips the tilt); the other two residues are twisted, h00 + h11 - h10 - h01 =
             +-0.75 m, so the wrong triangle or the wrong diagonal moves the depth by centimetres
  wall       i in [120, 123]: 896 (3.5 m)
  pit        i in [140, 160], j in [24, 40]: -256 (-1 m)
  target     i in [500, 511]: 2176 + 16 (j - 32), 6.5 .. 10.4 m, on the high x edge

A row is posed in one of three ways:
  q    one of the twelve rotations whose quaternion components lie in {0, +-1/2, +-1}, camera pitch 0:
       the direction is +-x, +-y or +-z bit for bit on host and device
  ypr  base yaw and roll (quat_from_euler, rounded to float32) and camera pitch: D = Rz(yaw) Rx(roll) Ry(pitch) e_x
  ray  a direct direction (exactly diagonal rays, rays pitched inside an edge's plane): host march only

Margins (tests/test_depth_cases.py::test_table_keeps_its_promises checks them in float64):
  * every hit row's |dg/dt| along the unit direction is >= 0.1 (no grazing hit); the two rows whose
    origin lies on the surface (t = 0 for every direction) are the stated exception
  * every ypr row's reference depth moves by < 1e-3 m when yaw and pitch move by +-1e-4 rad; q rows
    have no direction rounding, and those not lying in the field's boundary are held to it all the same
  * rows tagged "nd" (non-degenerate) keep origin and hit point >= 0.02 cells from every grid line and
    every diagonal
  * no row is left out of any comparison
"""
import types

import numpy as np

import depth_ref as DR

HS, VS, BORDER = 0.25, 2.0 ** -8, 4.0
NROWS, NCOLS = 512, 64
FOV = 10.0      # degrees: |d|max = 1.0076 at 1 x 1, so the geometric arm of the trip bound is 574 at far = 100
FAR = 8.0


def X(i):
    return i * HS - BORDER


Y = X


def field():
    """int16 [512, 64]."""
    i, j = np.meshgrid(np.arange(NROWS), np.arange(NCOLS), indexing="ij")
    h = np.full((NROWS, NCOLS), 128, np.int64)
    kerb = (i <= 6) & (j >= 44)
    h[kerb] = (128 + 16 * (j - 44))[kerb]
    slope = (i >= 40) & (i <= 80)
    h[slope] = (128 + 8 * (i - 40) + 4 * j)[slope]
    sad = (i >= 90) & (i <= 110) & (j >= 16) & (j <= 48)
    h[sad] = (128 + 64 * np.array([0, 1, -1])[(i - j) % 3])[sad]
    h[(i >= 120) & (i <= 123)] = 896
    h[(i >= 140) & (i <= 160) & (j >= 24) & (j <= 40)] = -256
    tgt = i >= 500
    h[tgt] = (2176 + 16 * (j - 32))[tgt]
    return h.astype(np.int16)


def scene():
    return DR.scene(field(), HS, VS, BORDER)


# ---- the twelve exact rotations, by where they send the camera's x axis
def _exact_quats():
    out = {}
    cands = [(0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (1, 0, 0, 0)]
    cands += [(sx * .5, sy * .5, sz * .5, .5) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    names = {(1, 0, 0): "+x", (-1, 0, 0): "-x", (0, 1, 0): "+y", (0, -1, 0): "-y", (0, 0, 1): "+z", (0, 0, -1): "-z"}
    for q in cands:
        ex = tuple(int(v) for v in DR._rot(q, np.float64)[:, 0])
        out.setdefault(names[ex], tuple(float(v) for v in q))
    assert len(out) == 6
    return out


QUATS = _exact_quats()
AXES = {"+x": (1., 0., 0.), "-x": (-1., 0., 0.), "+y": (0., 1., 0.), "-y": (0., -1., 0.), "+z": (0., 0., 1.), "-z": (0., 0., -1.)}


def _dir(yaw, pitch, roll=0.0):
    """Rz(yaw) Rx(roll) Ry(pitch) e_x: the base's yaw and roll, then the camera's pitch."""
    x, y, z = np.cos(pitch), np.sin(roll) * np.sin(pitch), -np.cos(roll) * np.sin(pitch)
    return np.array([np.cos(yaw) * x - np.sin(yaw) * y, np.sin(yaw) * x + np.cos(yaw) * y, z])


def _aim(ci, cj, z, yaw, pitch, dist, roll=0.0):
    """Origin `dist` before the point (X(ci), Y(cj), z) along the ypr direction, rounded to 2^-10 m."""
    o = np.array([X(ci), Y(cj), z]) - dist * _dir(yaw, pitch, roll)
    return tuple(np.round(o * 1024) / 1024)


def _row(name, o, q=None, ypr=None, ray=None, far=FAR, tags=(), kind="field", hit=True, at=None, cut=None):
    """at = (i, j, 'L' | 'U'): the cell and triangle the hit must lie in; cut: None, or 'before' / 'after' /
    'none' — where the hit lies relative to the ray's crossing of the hit cell's diagonal."""
    assert (q is not None) + (ypr is not None) + (ray is not None) == 1
    return types.SimpleNamespace(name=name, o=tuple(float(v) for v in o), q=q, ypr=ypr, ray=ray, far=float(far),
                                 tags=frozenset(tags), kind=kind, hit=hit, at=at, cut=cut)


PI = float(np.pi)
NAN = float("nan")
LVL = (1.1, 1.3)   # a point of the level zone, (u, v) = (20.4, 21.2)

ROWS = [
    # ---- which triangle (twisted cell (97, 30): lower 0.75 - 0.5 u + 0.5 v, upper 0.75 + 0.25 u - 0.25 v)
    _row("tri_lower_down", (20.4375, 3.5625, 1.0), q="-z", tags=("exact",), at=(97, 30, "L")),
    _row("tri_upper_down", (20.3125, 3.6875, 1.0), q="-z", tags=("exact",), at=(97, 30, "U")),
    _row("tri_lower_oblique", _aim(97.7, 30.3, 0.55, 0.6, 1.0, 1.1, 0.2), ypr=(0.6, 1.0, 0.2), tags=("nd",), at=(97, 30, "L")),
    _row("tri_upper_oblique", _aim(97.3, 30.7, 0.65, -2.1, 1.1, 1.0, -0.3), ypr=(-2.1, 1.1, -0.3), tags=("nd",), at=(97, 30, "U")),
    # ---- the diagonal cut
    _row("cut_hit_before", (19.8125, 3.625, 0.7), q="+x", at=(97, 30, "U"), cut="before"),
    _row("cut_hit_after_from_below", (20.275, 3.625, 0.55), q="+x", at=(97, 30, "L"), cut="after"),
    _row("cut_hit_after_oblique", _aim(97.8, 30.5, 0.6, 0.3, 1.2, 0.9), ypr=(0.3, 1.2, 0.0), tags=("nd",), at=(97, 30, "L"),
         cut="after"),
    # the cut past the stretch's midpoint and the hit after it: without the cut the whole stretch takes the
    # upper triangle's plane (v = 0.8: upper 0.55 + 0.25 u up to u = 0.8, lower 1.15 - 0.5 u after it)
    _row("cut_late_hit_after", _aim(97.925, 30.8, 0.6875, 0.0, 1.3, 0.5), ypr=(0.0, 1.3, 0.0), at=(97, 30, "L"), cut="after"),
    _row("cut_none_oblique", _aim(97.7, 30.3, 0.55, 0.9, 1.0, 0.8), ypr=(0.9, 1.0, 0.0), tags=("nd",), at=(97, 30, "L"),
         cut="none"),
    # ---- the two-sided rule, and g == 0 at a segment start
    _row("hit_from_above", LVL + (1.2,), ypr=(1.0, 0.5, -0.1), tags=("nd",)),
    _row("hit_from_below", LVL + (0.1,), ypr=(2.0, -0.8, 0.0), tags=("nd",)),
    _row("gs_zero_origin_on_surface", LVL + (0.5,), ypr=(0.4, 0.6, 0.0), tags=("exact", "onsurface")),
    # the level zone after the wall starts at X(124) = 27: the origin lies on that grid line, on the
    # level surface, and looks along it; the wall's last cell (not coplanar) touches the origin, so the
    # reference, which has no rule for a coplanar ray, returns 0 as well
    _row("in_level_surface", (27.0, 1.3, 0.5), q="+x", tags=("exact", "onsurface")),
    # ---- axis-parallel rays
    _row("dgx_zero_along_y", (-3.1, 7.0, 0.78125), q="+y", at=(3, 48, "L")),
    _row("dgy_zero_along_x", (25.1, 1.3, 1.2), q="+x"),           # the wall's rising face
    _row("dgy_zero_pitched", LVL + (1.2,), ypr=(0.0, 0.4, 0.0)),
    _row("straight_down", LVL + (0.75,), q="-z", tags=("exact",)),
    _row("straight_up_from_pit", (33.1, 3.3, -1.5), q="+z", tags=("exact",)),
    # ---- dgx == dgy (direct rays: host march only)
    _row("ddiag_zero_off_diagonal", LVL + (1.2,), ray=(0.5, 0.5, -0.5)),
    _row("ddiag_zero_on_diagonal_through_vertices", (20.125, 3.625, 0.9), ray=(0.5, 0.5, -0.25), tags=("vertices",)),
    _row("antidiagonal_through_vertices", (20.125, 3.625, 1.3), ray=(0.5, -0.5, -0.25), tags=("vertices",)),
    # ---- the origin on a grid line, moving backwards; on a vertex
    _row("origin_on_gridline_minus_x", (X(98), 3.55, 1.2), ypr=(2.8, 0.9, 0.0)),
    _row("origin_on_gridline_minus_y", (20.3, Y(32), 1.2), ypr=(-1.9, 0.9, 0.0)),
    _row("origin_on_vertex_down", (X(97), Y(30), 1.0), q="-z", tags=("exact",)),
    _row("origin_on_vertex_oblique", (X(99), Y(32), 1.3), ypr=(-2.5, 0.9, 0.0)),
    # ---- the extent: inside looking out (nothing), outside looking in, outside and missing
    _row("inside_out_low_x", (-3.7, 1.3, 1.0), ypr=(PI, 0.3, 0.0), hit=False),
    _row("inside_out_high_x", (123.45, 2.3, 9.0), ypr=(0.0, 0.3, 0.0), hit=False),
    _row("inside_out_low_y", (1.1, -3.7, 1.0), ypr=(-PI / 2, 0.3, 0.0), hit=False),
    _row("inside_out_high_y", (1.1, 11.45, 1.0), ypr=(PI / 2, 0.3, 0.0), hit=False),
    _row("outside_in_low_x", (-5.0, 1.3, 1.5), ypr=(0.2, 0.5, 0.0)),
    _row("outside_in_high_x", (124.5, 2.3, 12.0), ypr=(PI - 0.1, 1.1, 0.0)),
    _row("outside_in_low_y", (1.1, -5.0, 1.5), ypr=(PI / 2 - 0.2, 0.5, 0.0)),
    _row("outside_in_high_y", (1.1, 12.75, 1.5), ypr=(-PI / 2 + 0.2, 0.5, 0.0)),
    # hits inside the cell it enters by, on the slope (the gap is linear from t0 on, not from t = 0)
    _row("outside_in_hit_in_entry_cell", (8.1, -4.3, 1.27), ypr=(PI / 2 - 0.1, 1.0, 0.0), at=(48, 0, "L")),
    _row("outside_in_axis_low_x", (-5.0, 8.125, 0.6), q="+x"),     # enters under the kerb, leaves it from below
    _row("miss_outside", (-6.0, -6.0, 1.0), ypr=(2.5, 0.3, 0.0), hit=False),
    _row("miss_axis_parallel_y_outside", (-6.0, -5.0, 1.0), q="+x", hit=False),   # dgy == 0, v0 < 0: t1 = -1
    _row("miss_axis_parallel_x_outside", (124.0, -5.0, 1.0), q="+y", hit=False),  # dgx == 0, u0 > rows - 1
    # ---- the closed boundary: the high edges (each misses before the fix) and their low mirrors
    _row("edge_down_high_u", (X(511), 2.375, 8.5), q="-z", tags=("exact", "boundary", "high")),
    _row("edge_down_low_u", (X(0), 2.375, 0.75), q="-z", tags=("exact", "boundary")),
    _row("edge_down_high_v", (1.125, Y(63), 0.75), q="-z", tags=("exact", "boundary", "high")),
    _row("edge_down_low_v", (1.125, Y(0), 0.75), q="-z", tags=("exact", "boundary")),
    _row("edge_down_high_corner", (X(511), Y(63), 10.75), q="-z", tags=("exact", "boundary", "high")),
    _row("edge_down_low_corner", (X(0), Y(0), 0.75), q="-z", tags=("exact", "boundary")),
    _row("edge_along_high_u", (X(511), -1.375, 8.21875), q="+y", tags=("boundary", "high")),
    _row("edge_along_low_u", (X(0), 1.125, 0.78125), q="+y", tags=("boundary",)),
    _row("edge_along_high_v", (1.125, Y(63), 1.5), q="+x", tags=("boundary", "high")),
    _row("edge_along_low_v", (1.125, Y(0), 0.828125), q="+x", tags=("boundary",)),
    _row("edge_along_high_u_pitched", (X(511), -1.375, 9.5), ray=(0.0, 0.5, -0.25), tags=("boundary", "high")),
    _row("edge_along_low_u_pitched", (X(0), 1.125, 1.5), ray=(0.0, 0.5, -0.25), tags=("boundary",)),
    _row("edge_along_high_v_pitched", (1.125, Y(63), 1.5), ray=(0.5, 0.0, -0.25), tags=("boundary", "high")),
    _row("edge_along_low_v_pitched", (1.125, Y(0), 1.5), ray=(0.5, 0.0, -0.25), tags=("boundary",)),
    # on the target's surface on the high x edge, looking out of the field: the boundary point itself is hit
    _row("edge_origin_on_surface_high_u_outward", (X(511), 2.375, 8.09375), ypr=(0.0, 0.5, 0.0),
         tags=("exact", "onsurface", "boundary", "high")),
    _row("edge_origin_high_u_inward", (X(511), 2.3, 9.0), ypr=(PI - 0.3, 1.0, 0.0)),
    # ---- far
    _row("hit_beyond_far", LVL + (9.0,), q="-z", hit=False),
    _row("hit_exactly_at_far", LVL + (8.5,), q="-z", tags=("exact",)),
    # ---- long rows, all ending on the target wall (or the wall) at a level height
    _row("long_x_far100_geo_arm", (24.125, 1.3, 4.0), q="+x", far=100.0, tags=("long", "trip")),
    _row("long_oblique_far100_geo_arm", (24.125, 1.3, 4.0), ypr=(0.05, 0.0, 0.0), far=100.0, tags=("long", "trip")),
    _row("long_x_far120_extent_arm", (1.125, 1.3, 4.0), q="+x", far=120.0, tags=("long", "trip")),
    # from the low x edge to the target across 22 columns: 522 cells, more than the field has rows
    _row("long_oblique_far130_extent_arm", (-3.875, 1.3, 4.0), ypr=(0.045, 0.0, 0.0), far=130.0, tags=("long", "trip")),
    _row("long_origin_beyond_100m_back", (110.125, 1.3, 1.5), q="-x", far=120.0, tags=("long", "trip")),
    _row("long_origin_beyond_100m", (104.125, 1.3, 4.0), ypr=(0.1, 0.0, 0.0), far=100.0, tags=("long",)),
    # ---- guards: each gives far_clip
    _row("guard_nan_position", (NAN, 1.3, 1.0), q="-z", tags=("guard",), hit=False),
    _row("guard_nan_pitch", LVL + (1.0,), ypr=(0.0, NAN, 0.0), tags=("guard",), hit=False),
    _row("guard_zero_quaternion", LVL + (1.0,), q="zero", tags=("guard",), hit=False),
    _row("guard_origin_1e6_cells_away", (3.0e5, 1.3, 1.0), q="-x", tags=("guard",), hit=False),
    # ---- the plane z = 0 (terrain_type == 0)
    _row("plane_from_above", (1.0, 2.0, 1.2), ypr=(0.3, 0.5, 0.1), kind="plane"),
    _row("plane_from_below", (1.0, 2.0, -0.7), ypr=(0.3, -0.6, 0.0), kind="plane"),
    _row("plane_dz_zero_above", (1.0, 2.0, 1.0), q="+x", kind="plane", hit=False),
    _row("plane_above_looking_up", (1.0, 2.0, 1.2), ypr=(0.3, -0.5, 0.0), kind="plane", hit=False),   # th < 0
    _row("plane_oz_zero",(1.0, 2.0, 0.0), ypr=(0.3, 0.5, 0.0), kind="plane", tags=("exact", "onsurface")),
    _row("plane_straight_down", (1.0, 2.0, 1.25), q="-z", kind="plane", tags=("exact",)),
    _row("plane_hit_beyond_far", (1.0, 2.0, 9.0), q="-z", kind="plane", hit=False),
]

QUATS["zero"] = (0.0, 0.0, 0.0, 0.0)

# every branch the table promises (a prefix of at least one row's name)
BRANCHES = [
    "tri_lower", "tri_upper", "cut_hit_before", "cut_hit_after", "cut_none", "hit_from_above", "hit_from_below",
    "gs_zero", "in_level_surface", "dgx_zero", "dgy_zero", "straight_down", "straight_up", "ddiag_zero_off_diagonal",
    "ddiag_zero_on_diagonal", "antidiagonal_through_vertices", "origin_on_gridline_minus_x", "origin_on_gridline_minus_y",
    "origin_on_vertex", "inside_out_low_x", "inside_out_high_x", "inside_out_low_y", "inside_out_high_y",
    "outside_in_low_x", "outside_in_high_x", "outside_in_low_y", "outside_in_high_y", "miss_outside", "miss_axis_parallel",
    "edge_down_high_u", "edge_down_low_u", "edge_down_high_v", "edge_down_low_v", "edge_down_high_corner",
    "edge_down_low_corner", "edge_along_high_u", "edge_along_low_u", "edge_along_high_v", "edge_along_low_v",
    "hit_beyond_far", "hit_exactly_at_far", "long_x_far100_geo_arm", "long_x_far120_extent_arm", "long_origin_beyond_100m",
    "guard_nan_position", "guard_nan_pitch", "guard_zero_quaternion", "guard_origin_1e6", "plane_from_above",
    "plane_from_below", "plane_dz_zero", "plane_above_looking_up", "plane_oz_zero", "plane_hit_beyond_far",
]

# the rows the parent's march (no closed boundary) gets wrong: exactly these
HIGH_EDGE = [r.name for r in ROWS if "high" in r.tags]

CAM = DR.camera(1, 1, FOV, (0.0, 0.0, 0.0))


def pose(row):
    """(root [13] float32, camera pitch float32) of a q / ypr row; None for a direct ray."""
    if row.ray is not None:
        return None
    root = np.zeros(13, np.float64)
    root[:3] = row.o
    if row.q is not None:
        root[3:7], pitch = QUATS[row.q], 0.0
    else:
        yaw, pitch, roll = row.ypr
        root[3:7] = DR.quat_from_euler(roll, 0.0, yaw)
    return root.astype(np.float32), np.float32(pitch)


def ray64(row, dyaw=0.0, dpitch=0.0):
    """Origin and direction in float64: of the float32 pose (what the device is given), or the direct
    ray rounded to float32.  dyaw / dpitch perturb a ypr or q row's direction (the margin test)."""
    if row.ray is not None:
        return np.asarray(np.float32(row.o), np.float64), np.asarray(np.float32(row.ray), np.float64)
    root, pitch = pose(row)
    root = root.astype(np.float64)
    if dyaw:
        cz, sz = np.cos(dyaw / 2), np.sin(dyaw / 2)
        x, y, z, w = root[3:7]
        root[3:7] = (cz * x - sz * y, cz * y + sz * x, cz * z + sz * w, cz * w - sz * z)   # Rz(dyaw) q
    with np.errstate(invalid="ignore", divide="ignore"):
        o, D = DR.rays(types.SimpleNamespace(W=1, H=1, fov=FOV, pos=(0.0, 0.0, 0.0), far=row.far), root,
                       np.float64(pitch) + dpitch, ((0.0, 0.0),), np.float64)
    return o, D[0, 0, 0]


def reference(row, sc, dtype=np.float64, dyaw=0.0, dpitch=0.0):
    """The reference depth of one row (tests/depth_ref.py), all arithmetic in dtype."""
    o, D = ray64(row, dyaw, dpitch)
    return reference_ray(row.kind, sc, o, D, row.far, dtype)


def reference_ray(kind, sc, o, D, far, dtype=np.float64):
    dtype = np.dtype(dtype).type
    o, D, far = np.asarray(o).astype(dtype), np.asarray(D).astype(dtype), dtype(far)
    if kind == "plane":
        if not (np.isfinite(o).all() and np.isfinite(D).all()):
            return float(far)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[2] / D[2]
        return float(t if np.isfinite(t) and 0 <= t <= far else far)
    with np.errstate(invalid="ignore"):
        return float(DR._rays_field(sc, o, D[None, :], far, dtype)[0])


def height64(hf, u, v):
    """ground()'s surface in float64 at grid coordinates (u, v) inside the closed extent."""
    i, j = min(int(np.floor(u)), hf.shape[0] - 2), min(int(np.floor(v)), hf.shape[1] - 2)
    a, b = u - i, v - j
    h00, h10, h01, h11 = (VS * float(hf[i + di, j + dj]) for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)))
    return h00 + a * (h10 - h00) + b * (h11 - h10) if a >= b else h00 + b * (h01 - h00) + a * (h11 - h01)


def trip_bound(far, fov_deg=FOV, W=1, H=1, rows=NROWS, cols=NCOLS, hs=HS):
    """hg_launch_depth's trip count, restated: (bound, geo, ext)."""
    tan_h = np.tan(0.5 * float(np.float32(fov_deg)) * (np.pi / 180.0))
    dmax = np.sqrt(1.0 + tan_h * tan_h * (1.0 + (H / W) * (H / W)))
    geo = np.ceil(float(np.float32(far)) * dmax / float(np.float32(hs)) * 1.4142135623730951) + 4.0
    ext = float(rows) + float(cols) + 4.0
    return max(int(min(geo, ext)), 1), int(geo), int(ext)
