"""The depth march on planted rays, without a GPU: depth_march (csrc/hg_depth.hip, __host__
__device__) compiled for the host through tests/depth_host_shim.hip and run over the table of
tests/depth_cases.py against the float64 reference of tests/depth_ref.py.

The bound is the derivation of tests/test_depth_ref.py's SLACK, measured on the table itself: 8 x the
largest deviation of the reference's own float32 replay from its float64 values (4 x for an
independent float32 build, doubled because the march's formulation differs from the reference's).
Ordinary rows: measured 1.192e-7 m, held as REPLAY_DEV_ORD.  Long rows (far >= 100 m, origins beyond
100 m, where a float32 ulp is 8-15 um): measured 4.486e-6 m, held as REPLAY_DEV_LONG.
test_replay_stays_inside_the_constants prints both.
"""
import ctypes
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import depth_cases as DC
import depth_ref as DR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "humanoid-gym-with-comments_amd", "csrc")
SHIM = os.path.join(REPO, "tests", "depth_host_shim.hip")

REPLAY_DEV_ORD = 1.2e-7     # metres: float32 replay of the reference, ordinary rows (measured 1.192e-7)
REPLAY_DEV_LONG = 4.5e-6    # metres: the same on the long rows alone (measured 4.486e-6)
BOUND_ORD = 8 * REPLAY_DEV_ORD
BOUND_LONG = 8 * REPLAY_DEV_LONG

f32 = np.float32


def bound(row):
    return BOUND_LONG if "long" in row.tags else BOUND_ORD


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _compile(out_dir, name, src=None):
    """The shim around `src` (default: the tree's hg_depth.hip) as a shared object; nothing is launched,
    but the fat-binary symbols resolve only in a full (host + gfx950) build."""
    so = os.path.join(str(out_dir), f"depth_host_{name}.so")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-O3", "-std=c++17", "-I", CSRC, SHIM, "-o", so]
    if src is not None:
        cmd.insert(1, f'-DHG_DEPTH_SRC="{src}"')
    subprocess.run(cmd, check=True, capture_output=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.depth_march_host.restype = None
    L.depth_march_host.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_float, vp, vp, vp, vp]
    return L


def march(L, hf, hs, vs, border, o, D, far, steps):
    """depth_march on rays o [n, 3], D [n, 3] (rounded to float32), far [n], steps [n]; hf None = the plane."""
    n = len(o)
    ray = np.zeros((n, 8), f32)
    ray[:, 0:2], ray[:, 4], ray[:, 5:8] = np.asarray(o)[:, :2], np.asarray(o)[:, 2], D
    far = np.ascontiguousarray(np.broadcast_to(np.asarray(far, f32), (n,)))
    steps = np.ascontiguousarray(np.broadcast_to(np.asarray(steps, np.int32), (n,)))
    out = np.full(n, -7.0, f32)
    if hf is None:
        rows = cols = 0
        hfp = None
    else:
        hf = np.ascontiguousarray(hf, np.int16)
        rows, cols = hf.shape
        hfp = hf.ctypes.data
    L.depth_march_host(n, int(hf is not None), hfp, rows, cols, f32(hs), f32(vs), f32(border), ray.ctypes.data,
                       far.ctypes.data, steps.ctypes.data, out.ctypes.data)
    return out


class Table:
    """The table's rays as the march is given them (float32 origin and direction) and the float64
    reference at exactly those rays (computed once)."""

    def __init__(self):
        self.sc = DC.scene()
        self.rows = DC.ROWS
        self.o, self.D = [], []
        for r in self.rows:
            o, D = DC.ray64(r)
            self.o.append(f32(o))
            self.D.append(f32(D))
        self.o, self.D = np.asarray(self.o), np.asarray(self.D)
        self.far = np.asarray([r.far for r in self.rows], f32)
        self.field = np.asarray([r.kind == "field" for r in self.rows])
        self.ref = np.asarray([DC.reference_ray(r.kind, self.sc, self.o[k].astype(np.float64), self.D[k].astype(np.float64),
                                                r.far) for k, r in enumerate(self.rows)])

    def run(self, L, steps=None):
        if steps is None:
            steps = np.asarray([DC.trip_bound(r.far)[0] if r.kind == "field" else 1 for r in self.rows], np.int32)
        steps = np.broadcast_to(np.asarray(steps, np.int32), (len(self.rows),))
        out = np.empty(len(self.rows), f32)
        for sel, hf in ((self.field, self.sc.hf), (~self.field, None)):
            out[sel] = march(L, hf, DC.HS, DC.VS, DC.BORDER, self.o[sel], self.D[sel], self.far[sel], steps[sel])
        return out

    def failures(self, got):
        """Names of the rows a march's depths fail: outside the row's bound, or, on exact and guard
        rows, any other bits than the reference's."""
        bad = []
        for k, r in enumerate(self.rows):
            strict = "exact" in r.tags or "guard" in r.tags
            ok = (got[k] == self.ref[k]) if strict else (abs(float(got[k]) - self.ref[k]) <= bound(r))
            if not ok:
                bad.append(r.name)
        return bad


@pytest.fixture(scope="module")
def table():
    return Table()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    return _compile(tmp_path_factory.mktemp("depth_host"), "tree")


# ---------------------------------------------------------------- the table's promises
def _hit_geometry(row, sc, t):
    """(u, v) at the hit, (u, v) where the ray enters the hit's cell (or starts), the cell, in float64."""
    o, D = DC.ray64(row)
    gu = lambda s: ((o[0] + s * D[0] + DC.BORDER) / DC.HS, (o[1] + s * D[1] + DC.BORDER) / DC.HS)  # noqa: E731
    u, v = gu(t)
    i, j = min(int(np.floor(u)), DC.NROWS - 2), min(int(np.floor(v)), DC.NCOLS - 2)
    tin = 0.0
    for c, d, lo in ((u, D[0] / DC.HS, i), (v, D[1] / DC.HS, j)):
        if d != 0:
            back = (c - (lo if d > 0 else lo + 1)) / d     # time since the ray crossed into the cell on this axis
            tin = max(tin, t - back)
    return (u, v), gu(max(tin, 0.0)), (i, j)


def _dg_dt(row, sc, t):
    """d gap / d arclength just before the hit, one-sided over 1e-4 m, in float64."""
    o, D = DC.ray64(row)
    n = np.linalg.norm(D)
    g = lambda s: o[2] + s * D[2] - DC.height64(sc.hf, (o[0] + s * D[0] + DC.BORDER) / DC.HS,   # noqa: E731
                                                 (o[1] + s * D[1] + DC.BORDER) / DC.HS)
    ds = 1e-4 / n
    return (g(t) - g(t - ds)) / 1e-4


def test_table_keeps_its_promises(table):
    rows, sc = table.rows, table.sc
    names = [r.name for r in rows]
    assert len(set(names)) == len(names)
    for b in DC.BRANCHES:
        assert any(n.startswith(b) for n in names), f"no row for branch {b}"
    hf = sc.hf
    assert hf.shape == (DC.NROWS, DC.NCOLS) and hf.dtype == np.int16 and DC.NROWS != DC.NCOLS
    assert DC.X(DC.NROWS - 1) > 100.0 + DC.X(0)
    # saddle cells as stated: the tilted (0, +a, -a, 0) kind and the twisted kind
    c = hf[96:98, 30:32].astype(int)
    assert c[0, 0] == c[1, 1] and c[1, 0] - c[0, 0] == -(c[0, 1] - c[0, 0]) == 64
    c = hf[97:99, 30:32].astype(int)
    assert abs(c[0, 0] + c[1, 1] - c[1, 0] - c[0, 1]) * DC.VS >= 0.5
    c = hf[50:52, 10:12].astype(int)
    assert c[0, 0] + c[1, 1] - c[1, 0] - c[0, 1] == 0 and c[1, 0] != c[0, 0] and c[0, 1] != c[0, 0]   # the slope: coplanar
    assert hf.min() < 0
    worst_move, least_slope = 0.0, np.inf
    for k, r in enumerate(rows):
        ref = DC.reference(r, sc)          # at the float32 pose: what the GPU test compares with
        assert (ref < r.far or ("exact" in r.tags and ref == r.far)) == r.hit, f"{r.name}: reference {ref}, far {r.far}"
        if "guard" in r.tags:
            assert ref == r.far
            continue
        if "exact" in r.tags:
            assert float(f32(ref)) == ref, f"{r.name}: {ref!r} is no float32"
        # direction margin: every posed row but those lying in the field's boundary (their direction is exact)
        if r.ray is None and "boundary" not in r.tags:
            for dy, dp in ((1e-4, 0), (-1e-4, 0), (0, 1e-4), (0, -1e-4)):
                move = abs(DC.reference(r, sc, dyaw=dy, dpitch=dp) - ref)
                worst_move = max(worst_move, move)
                assert move < 1e-3, f"{r.name}: moves {move:.2e} m under ({dy}, {dp}) rad"
        else:
            assert r.ray is not None or r.q is not None or "onsurface" in r.tags, r.name   # exact, or t = 0 whatever D
        if r.kind != "field" or not r.hit or ref >= r.far:
            continue
        (u, v), (ue, ve), (i, j) = _hit_geometry(r, sc, ref)
        if "onsurface" not in r.tags:
            s = abs(_dg_dt(r, sc, ref))
            least_slope = min(least_slope, s)
            assert s >= 0.1, f"{r.name}: grazing, |dg/dt| = {s:.3f}"
        if r.at is not None:
            assert (i, j) == r.at[:2], f"{r.name}: hits cell {(i, j)}"
            side = (u - i) - (v - j)
            assert abs(side) >= 0.02 and (side > 0) == (r.at[2] == "L"), f"{r.name}: u - v = {side:.3f}"
        if r.cut is not None:
            s_hit, s_in = (u - i) - (v - j), (ue - i) - (ve - j)
            o, D = DC.ray64(r)
            s_out = s_hit + (D[0] - D[1]) / DC.HS * 10.0     # far along the ray: does it cross the diagonal at all
            if r.cut == "after":
                assert s_hit * s_in < 0, r.name
            elif r.cut == "before":
                assert s_hit * s_in > 0 and s_hit * s_out < 0, r.name
            else:
                assert s_hit * s_in > 0, r.name
        if "nd" in r.tags:
            o, D = DC.ray64(r)
            for a, b in (((o[0] + DC.BORDER) / DC.HS, (o[1] + DC.BORDER) / DC.HS), (u, v)):
                fa, fb = a - np.floor(a), b - np.floor(b)
                assert min(fa, 1 - fa, fb, 1 - fb) >= 0.02 and abs(fa - fb) >= 0.02, f"{r.name}: ({a:.3f}, {b:.3f})"
        if "vertices" in r.tags:
            o, D = DC.ray64(r)
            ts = [s for s in np.arange(1, 40) * (DC.HS / abs(D[0])) / 2 if s < ref]    # half-cell steps from a cell centre
            through = [s for s in ts if abs(((o[0] + s * D[0] + DC.BORDER) / DC.HS) % 1) < 1e-9
                       and abs(((o[1] + s * D[1] + DC.BORDER) / DC.HS) % 1) < 1e-9]
            assert len(through) >= 2, f"{r.name}: passes {len(through)} vertices before the hit"
    print(f"table: {len(rows)} rows, largest move under +-1e-4 rad {worst_move:.2e} m, least |dg/dt| {least_slope:.3f}")
    for name in DC.HIGH_EDGE:
        assert name.startswith("edge_") and "_high_" in name


def test_replay_stays_inside_the_constants(table):
    """The reference's own float32 replay against its float64 values, at the rays the march is given."""
    dev = {"ord": 0.0, "long": 0.0}
    for k, r in enumerate(table.rows):
        if "guard" in r.tags:
            continue
        rep = DC.reference_ray(r.kind, table.sc, table.o[k], table.D[k], r.far, np.float32)
        key = "long" if "long" in r.tags else "ord"
        dev[key] = max(dev[key], abs(rep - table.ref[k]))
    print(f"float32 replay: ordinary rows {dev['ord']:.3e} m (held {REPLAY_DEV_ORD:.1e}), long rows {dev['long']:.3e} m "
          f"(held {REPLAY_DEV_LONG:.1e})")
    assert 0.5 * REPLAY_DEV_ORD <= dev["ord"] <= REPLAY_DEV_ORD      # the constants are the measurement, not a guess
    assert 0.5 * REPLAY_DEV_LONG <= dev["long"] <= REPLAY_DEV_LONG


# ---------------------------------------------------------------- the host march on the table
def test_host_march_on_every_row(table, host):
    got = table.run(host)
    err = np.abs(got.astype(np.float64) - table.ref)
    for k, r in enumerate(table.rows):
        print(f"{r.name:44s} ref {table.ref[k]:.9g} march {got[k]:.9g} err {err[k]:.2e}")
    long = np.asarray(["long" in r.tags for r in table.rows])
    print(f"host march: largest deviation {err[~long].max():.3e} m on ordinary rows (bound {BOUND_ORD:.1e}), "
          f"{err[long].max():.3e} m on long rows (bound {BOUND_LONG:.1e})")
    assert table.failures(got) == []
    exact = [k for k, r in enumerate(table.rows) if "exact" in r.tags]
    assert len(exact) >= 12 and all(got[k] == table.ref[k] for k in exact)


def test_trip_bound(table, host):
    """hg_launch_depth's bound, restated in Python, decides no row (100 000 trips give the same bits);
    the trip rows need every cell they cross: one trip fewer returns far.  Both arms of the bound occur."""
    got = table.run(host)
    assert np.array_equal(got, table.run(host, 100000))
    arms = set()
    for k, r in enumerate(table.rows):
        if "trip" not in r.tags:
            continue
        b, geo, ext = DC.trip_bound(r.far)
        arms.add("geo" if geo < ext else "ext")
        assert ("geo_arm" in r.name) == (geo < ext) or "beyond" in r.name
        o, D = table.o[k].astype(np.float64), table.D[k].astype(np.float64)
        cell = lambda s: np.floor((o[:2] + s * D[:2] + DC.BORDER) / DC.HS)   # noqa: E731
        need = 1 + int(np.abs(cell(table.ref[k]) - cell(0.0)).sum())
        print(f"{r.name}: crosses {need} cells, bound {b} (geo {geo}, ext {ext})")
        assert 300 <= need <= b
        one = lambda s: march(host, table.sc.hf, DC.HS, DC.VS, DC.BORDER, table.o[k:k + 1], table.D[k:k + 1], r.far, s)[0]  # noqa: E731
        assert one(need) == got[k] and got[k] < r.far and one(need - 1) == f32(r.far)
    assert arms == {"geo", "ext"}


# ---------------------------------------------------------------- wrong marches
# (name, the line replaced, its replacement, rows that must fail | the reason it is equivalent)
WRONG = [
    ("midpoint_lt", "fmaf(tm, dgx, u0) - fci >= fmaf(tm, dgy, v0) - fcj;", "fmaf(tm, dgx, u0) - fci < fmaf(tm, dgy, v0) - fcj;",
     ["tri_lower_down", "tri_upper_down", "tri_lower_oblique", "tri_upper_oblique"]),
    ("cut_never", "const bool cut = ddiag != 0.f && td > ts && td < te;", "const bool cut = false;",
     ["cut_hit_before", "cut_late_hit_after"]),
    ("p1_pC_swapped", "h01 = vs * p[1], h10 = vs * p[C]", "h01 = vs * p[C], h10 = vs * p[1]",
     ["tri_lower_down", "tri_upper_down", "dgx_zero_along_y", "dgy_zero_along_x"]),
    ("no_hit_from_below", "if ((gs >= 0.f && gd <= 0.f) || (gs <= 0.f && gd >= 0.f)) {", "if (gs >= 0.f && gd <= 0.f) {",
     ["hit_from_below", "straight_up_from_pit"]),
    ("vertex_steps_one_axis", "if (tx <= ty) ci += sx;", "if (tx < ty) ci += sx;", None),
    ("backward_cell_edge", "(float)(ci + (sx > 0))", "(float)(ci + 1)",
     ["origin_on_gridline_minus_x", "origin_on_gridline_minus_y", "long_origin_beyond_100m_back"]),
    ("start_at_zero", "float ts = t0;", "float ts = 0.f;", ["outside_in_hit_in_entry_cell"]),
    ("root_is_midpoint", "t = gs == gd ? ts : ts + (td - ts) * (gs / (gs - gd));", "t = gs == gd ? ts : 0.5f * (ts + td);",
     ["straight_down", "hit_from_above", "tri_lower_down"]),
    ("hix_one_short", "hix = (float)(rows - 1 - i0)", "hix = (float)(rows - 2 - i0)",
     ["edge_down_high_u", "edge_along_high_u", "edge_down_high_corner"]),
    ("plane_behind", "if (Dz != 0.f && th >= 0.f && th <= zfar) t = th;", "if (Dz != 0.f && th <= zfar) t = th;",
     ["plane_above_looking_up"]),
    ("parent_high_edge", "const bool ei = dgx >= 0.f && i0 + ci == rows - 1, ej = dgy >= 0.f && j0 + cj == C - 1;",
     "const bool ei = false, ej = false;",
     DC.HIGH_EDGE),
    ("no_carried_sign", "if (prev * sgn(gs) < 0) { t = ts; break; }", "if (false) { t = ts; break; }", None),
    ("no_u_clamp", "u = fminf(fmaxf(u, 0.f), 1.f);", "", None),
]

# what the None entries above turned out to be (recorded, not dropped): the reason each is equivalent
EQUIVALENT = {
    "vertex_steps_one_axis": "at a vertex only cj steps; the next trip is a zero-length segment in the side cell, whose two "
                             "gap values are one value (no crossing), after which ci steps: the same cells, one trip later",
    "no_carried_sign": "on the dyadic field both cells' expressions at a shared point are exact, so their signs agree; the "
                       "carried sign only acts on a rounding disagreement",
    "no_u_clamp": "segment ends are computed inside their cell to within rounding, and the table's heights are linear "
                  "in u, v; the clamp only guards an end point a few ulp outside the cell",
}


@pytest.fixture(scope="module")
def wrong(tmp_path_factory, host):
    out = tmp_path_factory.mktemp("depth_wrong")
    text = open(os.path.join(CSRC, "hg_depth.hip")).read()
    jobs = []
    for name, old, new, _ in WRONG:
        assert text.count(old) == 1, f"{name}: the replaced line matches {text.count(old)} times"
        src = os.path.join(str(out), f"hg_depth_{name}.hip")
        with open(src, "w") as f:
            f.write(text.replace(old, new))
        jobs.append((name, src))
    with ThreadPoolExecutor(4) as ex:
        libs = list(ex.map(lambda j: _compile(out, j[0], j[1]), jobs))
    return {name: L for (name, _), L in zip(jobs, libs)}


@pytest.mark.parametrize("name", [w[0] for w in WRONG])
def test_wrong_march_fails_the_table(table, wrong, name):
    expect = next(w[3] for w in WRONG if w[0] == name)
    bad = table.failures(table.run(wrong[name]))
    print(f"{name}: fails {bad}")
    if expect is None:
        assert name in EQUIVALENT and bad == [], f"{name} is recorded as equivalent but fails {bad}"
    else:
        assert set(expect) <= set(bad), f"{name}: passes {sorted(set(expect) - set(bad))}"
    if name == "parent_high_edge":
        assert sorted(bad) == sorted(DC.HIGH_EDGE)      # the parent fails exactly the high-edge rows


# ---------------------------------------------------------------- seeded fuzz
def _fuzz_fields():
    rs = np.random.RandomState(11)
    i, j = np.meshgrid(np.arange(48), np.arange(40), indexing="ij")
    steps = (64 * ((i // 6 + j // 5) % 4)).astype(np.int16)                         # level terraces with cliffs
    slope = (6 * i - 3 * j + 100).astype(np.int16)                                  # one plane
    saddle = (128 + 64 * np.array([0, 1, -1])[(i - j) % 3]).astype(np.int16)       # the table's saddles
    rough = rs.randint(-40, 41, size=(48, 40)).astype(np.int16)                     # decimetre noise
    return [steps, slope, saddle, rough]


def _fuzz_rays(rs, n, rows, cols):
    """Origins and directions, float32: two thirds general, one third from the degenerate classes."""
    o = np.stack([rs.uniform(-5.0, DC.X(rows - 1) + 1.0, n), rs.uniform(-5.0, DC.X(cols - 1) + 1.0, n),
                  rs.uniform(-0.5, 2.5, n)], axis=1)
    yaw, pit = rs.uniform(-np.pi, np.pi, n), np.deg2rad(rs.uniform(35.0, 90.0, n))   # no grazing rays: the reference
    D = np.stack([np.cos(yaw) * np.cos(pit), np.sin(yaw) * np.cos(pit), -np.sin(pit)], axis=1)   # would move under 1e-4 rad
    D[:, 2] *= np.where(o[:, 2] > 0.8, 1.0, rs.choice([-1.0, 1.0], n))
    general = np.ones(n, bool)
    for k in range(n):
        c = rs.randint(0, 18)
        if c >= 6:
            continue
        general[k] = False
        if c == 0:      # axis-parallel, pitched
            D[k, rs.randint(0, 2)] = 0.0
        elif c == 1:    # exactly diagonal or anti-diagonal
            D[k, 1] = D[k, 0] * rs.choice([-1.0, 1.0])
        elif c == 2:    # origin on a grid line or a vertex
            o[k, 0] = DC.X(rs.randint(0, rows))
            if rs.randint(0, 2):
                o[k, 1] = DC.X(rs.randint(0, cols))
        elif c == 3:    # straight down or up
            D[k] = (0.0, 0.0, -1.0 if o[k, 2] > 0.8 else rs.choice([-1.0, 1.0]))
        elif c == 4:    # on an edge of the field, in its plane (straight down half of the time)
            a = rs.randint(0, 2)
            o[k, a] = DC.X(rs.choice([0, (rows, cols)[a] - 1]))
            o[k, 2] = 2.0
            D[k, a] = 0.0
            if rs.randint(0, 2):
                D[k] = (0.0, 0.0, -1.0)
        else:           # from a cell centre along the diagonal: through vertices
            o[k, 0], o[k, 1] = DC.X(rs.randint(2, rows - 2)) + 0.125, DC.X(rs.randint(2, cols - 2)) + 0.125
            D[k, 0], D[k, 1] = 0.5, 0.5 * rs.choice([-1.0, 1.0])
    return o.astype(f32), D.astype(f32), general


def _turned(D, dyaw, dpitch):
    """D turned by dyaw about z and by dpitch in its own vertical plane (float64)."""
    c, s = np.cos(dyaw), np.sin(dyaw)
    D = np.array([c * D[0] - s * D[1], s * D[0] + c * D[1], D[2]])
    h = np.hypot(D[0], D[1])
    n = np.array([-D[2] * D[0] / h, -D[2] * D[1] / h, h]) if h > 1e-9 else np.array([np.linalg.norm(D), 0.0, 0.0])
    return D * np.cos(dpitch) + n * np.sin(dpitch)


def test_fuzz_against_the_reference(host):
    """4800 single rays over four small dyadic fields, far 8 m.  A general ray is left out only when the
    float64 reference itself moves by more than 1e-3 m under +-1e-4 rad (at most 0.5 % of the rays, a
    figure of the reference alone); the degenerate rays have exact directions and all stay in."""
    rs = np.random.RandomState(20261020)
    total = left_out = hits = 0
    worst = 0.0
    for hf in _fuzz_fields():
        sc = DR.scene(hf, DC.HS, DC.VS, DC.BORDER)
        o, D, general = _fuzz_rays(rs, 1200, *hf.shape)
        got = march(host, hf, DC.HS, DC.VS, DC.BORDER, o, D, DC.FAR, DC.trip_bound(DC.FAR, rows=hf.shape[0], cols=hf.shape[1])[0])
        o64, D64 = o.astype(np.float64), D.astype(np.float64)
        for k in range(len(o)):
            ref = DC.reference_ray("field", sc, o64[k], D64[k], DC.FAR)
            err = abs(float(got[k]) - ref)
            total += 1
            hits += ref < DC.FAR
            if general[k]:    # decided on the reference alone, before the march's value is looked at
                moves = max(abs(DC.reference_ray("field", sc, o64[k], _turned(D64[k], dy, dp), DC.FAR) - ref)
                            for dy, dp in ((1e-4, 0), (-1e-4, 0), (0, 1e-4), (0, -1e-4)))
                if moves > 1e-3:
                    left_out += 1
                    continue
            worst = max(worst, err)
            assert err <= BOUND_ORD, f"ray o = {o[k]!r}, D = {D[k]!r}: march {got[k]!r}, reference {ref!r}"
    assert hits >= 0.5 * total      # the rays see terrain
    print(f"fuzz: {total} rays, {hits} hit, {left_out} left out as unstable in the reference, largest deviation {worst:.3e} m")
    assert left_out <= 0.005 * total
