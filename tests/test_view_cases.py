"""The follow-camera view without a GPU: the __host__ __device__ intersection, nearest-shape and
shading functions of csrc/hg_view_shapes.h compiled for the host through tests/view_host_shim.hip
and run on planted rays against the float64 reference of tests/view_ref.py; the shape table against
its restatement; and the conditions that keep the GPU comparison (tests/test_gpu_view.py) honest.

Bounds.  Each is 8 x the largest deviation of the reference's own float32 replay from its float64
values (4 x for an independent float32 build, doubled because the kernel's formulation differs from
the reference's), measured by the test named beside it, printed there and held as a constant:
  RAY_REPLAY_DEV    the planted ray table          (test_replays_stay_inside_the_constants)
  FK_REPLAY_DEV     the planted poses' shape table (test_replays_stay_inside_the_constants)
  SCENE_REPLAY_DEV  centre pixels of the plane scenes (test_scene_set_keeps_the_gpu_test_honest)
  FIELD_REPLAY_DEV  centre pixels of the heightfield scenes (test_field_scenes_keep_the_gpu_test_honest);
                    held apart so that the field's coarser replay does not loosen the plane's slack
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_ref as DR
import view_ref as VR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "humanoid-gym-with-comments_amd", "csrc")
SHIM = os.path.join(REPO, "tests", "view_host_shim.hip")

RAY_REPLAY_DEV = 2.2e-7     # metres (measured 2.109e-7)
FK_REPLAY_DEV = 1.1e-5      # metres / quaternion units (measured 1.042e-5, at the env 180 m out)
SCENE_REPLAY_DEV = 6.2e-7   # metres: the plane scenes (measured 6.105e-7)
FIELD_REPLAY_DEV = 7.8e-5   # metres: the heightfield scenes (measured 7.744e-5, a thigh pixel near its silhouette)
RAY_BOUND = 8 * RAY_REPLAY_DEV
FK_BOUND = 8 * FK_REPLAY_DEV
SLACK = 8 * SCENE_REPLAY_DEV        # plane scenes
FIELD_SLACK = 8 * FIELD_REPLAY_DEV  # heightfield scenes (never applied to a plane scene)
UNDECIDED_CAP = 0.02

f32 = np.float32


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    so = os.path.join(str(tmp_path_factory.mktemp("view_host")), "view_host.so")
    subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-O3", "-std=c++17", "-I", CSRC, SHIM, "-o", so],
                   check=True, capture_output=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.view_ray_rows_host.restype = None
    L.view_ray_rows_host.argtypes = [ctypes.c_int, vp, vp, vp]
    L.view_nearest_host.restype = ctypes.c_int
    L.view_nearest_host.argtypes = [vp, vp, ctypes.c_int, ctypes.c_float, vp]
    L.view_shade_host.restype = None
    L.view_shade_host.argtypes = [ctypes.c_int, vp, vp]
    L.view_table_host.restype = ctypes.c_int
    L.view_table_host.argtypes = [vp, vp]
    return L


@pytest.fixture(scope="module")
def model():
    from humanoid import _native as N
    return N.load_model()[0]


# ---------------------------------------------------------------- the planted ray table
def _cap(p0, p1, r):
    row = np.zeros(16)
    row[0], row[1:4], row[4:7], row[7] = 0, p0, p1, r
    return row


def _box(c, h, q=(0, 0, 0, 1), kind=1):
    row = np.zeros(16)
    row[0], row[1:4], row[4:7], row[7:11] = kind, c, h, q
    return row


CAP = _cap((3, 0.2, -0.3), (3, 0.2, 0.4), 0.05)            # axis along z
SKEW = _cap((2.1, -0.4, 0.3), (2.6, 0.1, -0.2), 0.08)
BALL = _cap((2, -0.3, 0.1), (2, -0.3, 0.1), 0.07)          # p0 == p1
UNIT = _cap((3, 0, 0), (3, 0, 0), 1.0)                     # exact arithmetic: t = 2
BOX = _box((2, 0.5, 0.3), (0.2, 0.1, 0.15))
QROT = DR.quat_from_euler(0.3, -0.5, 1.1)
RBOX = _box((2.2, -0.6, 0.4), (0.2, 0.1, 0.15), QROT, kind=2)
NAN, INF = float("nan"), float("inf")
G = 1e-4  # the grazing rays' tangent offset, metres

# (name, row, origin, direction, far, tags) — tags: "graze" / "edge": the normal is not compared
ROWS = [
    ("cap axis through both caps", CAP, (3, 0.2, -2), (0, 0, 1), 10, ""),
    ("cap axis from above", CAP, (3, 0.2, 2), (0, 0, -1), 10, ""),
    ("cap perpendicular through the axis", CAP, (0, 0.2, 0), (1, 0, 0), 10, ""),
    ("cap perpendicular, direction not unit", CAP, (0, 0.2, 0.1), (2.5, 0, 0), 10, ""),
    ("cap grazing inside", CAP, (0, 0.2 + 0.05 - G, 0), (1, 0, 0), 10, "graze"),
    ("cap grazing outside", CAP, (0, 0.2 + 0.05 + G, 0), (1, 0, 0), 10, "graze"),
    ("cap parallel to the axis inside", CAP, (3.02, 0.21, -2), (0, 0, 1), 10, ""),
    ("cap parallel to the axis outside", CAP, (3.06, 0.2, -2), (0, 0, 1), 10, ""),
    ("cap hit beyond the segment end", CAP, (0, 0.2, 0.43), (1, 0, 0), 10, ""),
    ("cap miss beyond the segment end", CAP, (0, 0.2, 0.46), (1, 0, 0), 10, ""),
    ("cap oblique", CAP, (0.1, -0.2, 0.5), (1, 0.135, -0.17), 10, ""),
    ("skew oblique", SKEW, (0, 0, 0), (1, -0.07, 0.03), 10, ""),
    ("skew cap end", SKEW, (0, 0, 0), (1, 0.06, -0.1), 10, ""),
    ("sphere", BALL, (0, 0, 0), (1, -0.13, 0.06), 10, ""),
    ("sphere miss", BALL, (0, 0, 0), (1, -0.2, 0.06), 10, ""),
    ("cap origin inside", CAP, (3.01, 0.2, 0), (1, 0.3, 0), 10, ""),
    ("sphere origin inside", BALL, (2.02, -0.31, 0.1), (0, 1, 0), 10, ""),
    ("cap wholly behind", CAP, (5, 0.2, 0), (1, 0, 0), 10, ""),
    ("sphere hit exactly at far", UNIT, (0, 0, 0), (1, 0, 0), 2.0, ""),
    ("sphere just beyond far", UNIT, (0, 0, 0), (1, 0, 0), 1.9999, ""),
    ("box face centre", BOX, (0, 0.5, 0.3), (1, 0, 0), 10, ""),
    ("box edge approach", BOX, (1.0, -0.4, 0.3), (1, 1, 0), 10, "edge"),
    ("box corner approach", BOX, (1.3, -0.1, -0.35), (1, 1, 1), 10, "edge"),
    ("box parallel to a face inside the slab", BOX, (0, 0.55, 0.35), (1, 0, 0), 10, ""),
    ("box parallel to a face outside the slab", BOX, (0, 0.7, 0.3), (1, 0, 0), 10, ""),
    ("box oblique", BOX, (0.2, 0.1, 1.0), (1, 0.22, -0.4), 10, ""),
    ("box origin inside", BOX, (2.1, 0.45, 0.3), (0.3, 1, 0.2), 10, ""),
    ("box wholly behind", BOX, (3, 0.5, 0.3), (1, 0, 0), 10, ""),
    ("box hit beyond far", BOX, (0, 0.5, 0.3), (1, 0, 0), 1.7, ""),
    ("rotated box", RBOX, (0, 0, 0), (1, -0.27, 0.17), 10, ""),
    ("rotated box from above", RBOX, (2.1, -0.5, 2.0), (0.05, -0.04, -1), 10, ""),
    ("rotated box miss", RBOX, (0, 0, 0), (1, -0.5, 0.17), 10, ""),
    ("cap NaN origin", CAP, (NAN, 0.2, 0), (1, 0, 0), 10, ""),
    ("cap inf direction", CAP, (0, 0.2, 0), (INF, 0, 0), 10, ""),
    ("cap NaN direction", CAP, (0, 0.2, 0), (1, NAN, 0), 10, ""),
    ("box inf origin", BOX, (0, INF, 0.3), (1, 0, 0), 10, ""),
    ("box NaN direction", BOX, (0, 0.5, 0.3), (1, 0, NAN), 10, ""),
    ("rotated box NaN origin", RBOX, (0, 0, NAN), (1, -0.27, 0.17), 10, ""),
]
MUST_HIT = {"cap axis through both caps": 1.65, "cap perpendicular through the axis": 2.95, "sphere hit exactly at far": 2.0,
            "box face centre": 1.8, "box edge approach": 0.8, "box corner approach": 0.5, "cap origin inside": 0.0,
            "box origin inside": 0.0, "sphere origin inside": 0.0, "box parallel to a face inside the slab": 1.8}
MUST_MISS = ("cap grazing outside", "cap parallel to the axis outside", "cap miss beyond the segment end", "sphere miss",
             "cap wholly behind", "sphere just beyond far", "box parallel to a face outside the slab", "box wholly behind",
             "box hit beyond far", "rotated box miss")


def _rounded():
    rows = np.asarray([r[1] for r in ROWS], f32)
    ray = np.asarray([list(r[2]) + list(r[3]) + [r[4]] for r in ROWS], f32)
    return rows, ray


def _reference(dtype):
    """(hit [n] bool, t [n], normal [n, 3]) of the table's float32-rounded inputs, computed in dtype."""
    rows, ray = _rounded()
    hit, t, nrm = np.zeros(len(ROWS), bool), np.zeros(len(ROWS)), np.zeros((len(ROWS), 3))
    for k in range(len(ROWS)):
        row, o, d, far = rows[k].astype(np.float64), ray[k, 0:3], ray[k, 3:6], float(ray[k, 6])
        if row[0] == 0:
            tk, nk = VR.ray_capsule(o, d[None], row[1:4], row[4:7], row[7], far, dtype)
        else:
            tk, nk = VR.ray_box(o, d[None], row[1:4], row[4:7], DR._rot(row[7:11], np.float64), far, dtype)
        hit[k] = np.isfinite(tk[0]) and tk[0] <= far
        t[k], nrm[k] = (tk[0], nk[0]) if hit[k] else (0.0, 0.0)
    return hit, t, nrm


@pytest.fixture(scope="module")
def ref64():
    return _reference(np.float64)


def test_the_table_keeps_its_promises(ref64):
    hit, t, _ = ref64
    names = [r[0] for r in ROWS]
    for name, want in MUST_HIT.items():
        k = names.index(name)
        assert hit[k] and abs(t[k] - want) < 1e-6, (name, hit[k], t[k])
    for name in MUST_MISS:
        assert not hit[names.index(name)], name
    for k, r in enumerate(ROWS):
        if "NaN" in r[0] or "inf" in r[0]:
            assert not hit[k], r[0]
    assert hit[names.index("cap grazing inside")]


def test_replays_stay_inside_the_constants(ref64, model):
    hit, t, _ = ref64
    h32, t32, _ = _reference(np.float32)
    assert np.array_equal(hit, h32)
    dev = np.abs(t32 - t)[hit].max()
    fk = _fk_replay_dev(model)
    print(f"float32 replay: ray table {dev:.3e} m (held {RAY_REPLAY_DEV:.3e}), shape table of the planted poses "
          f"{fk:.3e} (held {FK_REPLAY_DEV:.3e})")
    assert dev <= RAY_REPLAY_DEV
    assert fk <= FK_REPLAY_DEV


def planted(model):
    return VR.planted_states(np.zeros(12), [model.lower[b] for b in range(1, 13)], [model.upper[b] for b in range(1, 13)])


def align_quats(tab, ref):
    """tab with every box row's quaternion given the sign of ref's (q and -q are one rotation)."""
    tab = np.array(tab, np.float64)
    flip = ((tab[..., 7:11] * ref[..., 7:11]).sum(-1) < 0) & (ref[..., 0] > 0)
    tab[..., 7:11] = np.where(flip[..., None], -tab[..., 7:11], tab[..., 7:11])
    return tab


def _fk_replay_dev(model):
    roots, q = planted(model)
    t64 = VR.table_array(VR.world_shapes(model, roots, q, np.float64))
    t32 = align_quats(VR.table_array(VR.world_shapes(model, roots, q, np.float32)), t64)
    return np.abs(t32 - t64).max()


def test_host_intersections_match_the_reference(host, ref64):
    hit, t, nrm = ref64
    rows, ray = _rounded()
    out = np.zeros((len(ROWS), 5), f32)
    host.view_ray_rows_host(len(ROWS), ray.ctypes.data, rows.ctypes.data, out.ctypes.data)
    bad = []
    for k, r in enumerate(ROWS):
        if bool(out[k, 0]) != hit[k]:
            bad.append((r[0], "hit", out[k, 0], hit[k]))
        elif hit[k]:
            if abs(float(out[k, 1]) - t[k]) > RAY_BOUND:
                bad.append((r[0], "t", out[k, 1], t[k]))
            # unit normals of ordinary rows: float32 directions agree to a few 1e-7 x the shape's
            # conditioning (distance / radius <= 60), far inside 1e-4
            if not r[5] and float(out[k, 2:5].astype(np.float64) @ nrm[k]) < 1 - 1e-4:
                bad.append((r[0], "normal", out[k, 2:5], nrm[k]))
    print(f"largest |t - ref| {max(abs(float(out[k, 1]) - t[k]) for k in range(len(ROWS)) if hit[k]):.3e} m "
          f"(bound {RAY_BOUND:.3e})")
    assert not bad, bad


def test_nearest_shape_rules(host):
    rows = np.asarray([BOX, CAP, CAP, BALL], f32)
    ray = np.asarray([0, 0.2, 0, 1, 0, 0], f32)
    t = ctypes.c_float(-1)
    call = lambda r, n, tmax: host.view_nearest_host(ray.ctypes.data, r.ctypes.data, n, tmax, ctypes.byref(t))  # noqa: E731
    assert call(rows, 4, 10.0) == 1 and abs(t.value - 2.95) < 1e-5       # two equal capsules: the lower index
    first = t.value
    assert call(rows, 4, first) == 1 and t.value == first               # a tie with the terrain goes to the shape
    assert call(rows, 4, np.nextafter(f32(first), f32(0))) == -1         # terrain nearer than every shape
    assert call(rows[3:], 1, 10.0) == -1                                 # nothing on the ray


def test_shading_matches_the_reference(host):
    rs = np.random.RandomState(3)
    n = 64
    inp = np.zeros((n, 9))
    inp[:, 0] = rs.randint(0, 5, n)
    inp[:, 1:3] = rs.uniform(-3, 3, (n, 2))
    inp[:8, 1:3] += 200.0
    inp[8:12, 1:3] = [[-0.25, 0.25], [-0.25, -0.25], [0.25, -1.75], [1.5, 2.5]]
    inp[8:12, 0] = 1
    v = rs.normal(size=(n, 3))
    inp[:, 3:6] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    inp[:, 6:9] = rs.normal(size=(n, 3)).astype(f32)
    out = np.zeros((n, 3), np.uint8)
    host.view_shade_host(n, inp.ctypes.data, out.ctypes.data)
    for k in range(n):
        cls = int(inp[k, 0])
        if cls == 0:
            want = 255.0 * np.array(VR.SKY)
        else:
            want = VR.shade(None if cls == 1 else cls - 2, inp[k, 1:3], inp[k, 3:6], inp[k, 6:9])
        assert np.abs(out[k].astype(np.float64) - np.rint(want)).max() <= 1, (k, cls, out[k], want)
    assert tuple(out[inp[:, 0] == 0][0]) == VR.SKY_U8 == (135, 181, 235)
    # the checker: floor, not truncation, left of the origin
    assert tuple(out[8]) != tuple(out[9])


def test_shape_table_matches_its_restatement(host, model):
    out = np.zeros((16, 9), f32)
    n = host.view_table_host(ctypes.byref(model), out.ctypes.data)
    want = VR.local_shapes(model)
    assert n == len(want) == 11
    assert [int(k) for k in out[:n, 0]] == [0] * 8 + [1, 1, 2]
    for s in range(n):
        kind, body, a, b, r = want[s]
        assert (int(out[s, 0]), int(out[s, 1])) == (kind, body)
        np.testing.assert_allclose(out[s, 2:5], a, rtol=0, atol=1e-7)
        np.testing.assert_allclose(out[s, 5:8], b, rtol=0, atol=1e-7)
        assert abs(out[s, 8] - r) < 1e-7
    # XBot-L's foot box (x +-0.0437, y -0.056 .. 0, z -0.074 .. 0.134) and base box (the 0.4 m cube 0.1 m up)
    lo, hi = out[8, 2:5] - out[8, 5:8], out[8, 2:5] + out[8, 5:8]
    np.testing.assert_allclose(lo, [-0.0437, -0.056, -0.074], atol=1e-4)
    np.testing.assert_allclose(hi, [0.0437, 0.0, 0.134], atol=1e-4)
    np.testing.assert_allclose(out[10, 2:8], [0, 0, 0.1, 0.2, 0.2, 0.2], atol=1e-6)
    assert [int(b) for b in out[8:11, 1]] == [6, 12, 0]


# ---------------------------------------------------------------- the scene set
def scene_refs(model):
    """[(name, env, cam, shapes64 of that env, base)] of the plane scene set."""
    roots, q = planted(model)
    sh = VR.world_shapes(model, roots, q, np.float64)
    return roots, q, [(name, e, cam, [sh[e]], [roots[e, :3]]) for name, e, cam in VR.plane_scenes(roots)]


def field_scenes(model):
    """The heightfield part of the scene set: planted envs 0 and 1 on the roughest cell of the suite's
    field under the long-lens follow camera at 64 x 36 (env 2, 180 m out, is the pose pass's and the
    plane's: at that distance the reference's own float32 triangle tests are the coarsest thing in the
    scene and would widen the slack fortyfold).  (scene, roots [2], dof_pos [2], [(name, cam)])."""
    hf, origins, tcfg = DR.terrain_field()
    sc = DR.field_scene(hf, tcfg)
    org = VR.rough_origin(sc, origins)
    roots, q = VR.planted_states(np.zeros(12), [model.lower[b] for b in range(1, 13)],
                                 [model.upper[b] for b in range(1, 13)], origin=org)
    roots, q = roots[:2], q[:2]
    return sc, roots, q, [("follow-64x36", VR.follow_camera(64, 36))]


def test_field_scenes_keep_the_gpu_test_honest(model):
    """As the plane scenes, for the follow camera over the heightfield; the deviation found here is
    part of SCENE_REPLAY_DEV."""
    sc, roots, q, cams = field_scenes(model)
    sh64 = VR.world_shapes(model, roots, q, np.float64)
    sh32 = VR.world_shapes(model, roots, q, np.float32)
    dev = 0.0
    for name, cam in cams:
        ref = VR.reference(sc, cam, sh64, roots[:, :3])
        rep = VR.render(sc, cam, sh32, roots[:, :3], dtype=np.float32)
        und = 1.0 - ref["decided"].reshape(len(roots), -1).mean(1)
        ad = np.abs(rep["t"][0].astype(np.float64) - ref["ctr"])
        d = ad.max()
        worst = np.unravel_index(ad.argmax(), ad.shape)
        print(f"{name}: worst pixel (env, row, col) {worst}: id {ref['idset'][0][worst]}, t {ref['ctr'][worst]:.6f}, "
              f"interval width {ref['hi'][worst] - ref['lo'][worst]:.3e}")
        dev = max(dev, d)
        fails = VR.failures(ref, rep["t"][0], rep["ids"][0], np.rint(rep["rgb"]), FIELD_SLACK)
        robot = (ref["idset"][0] >= 2).reshape(len(roots), -1).mean(1)
        terrain = (ref["idset"][0] == 1).reshape(len(roots), -1).mean(1)
        print(f"{name}: undecided {und}, robot {robot}, terrain {terrain}, replay deviation {d:.3e} m, failures {fails}")
        assert (und <= UNDECIDED_CAP).all(), name
        assert (robot >= 0.03).all() and (terrain >= 0.3).all(), name
        assert fails == (0, 0, 0), name
    print(f"field scenes: float32 replay centre deviation {dev:.3e} m (held {FIELD_REPLAY_DEV:.3e}, slack = 8 x)")
    assert dev <= FIELD_REPLAY_DEV


def test_outside_scene_keeps_the_gpu_test_honest(model):
    """The camera outside the field's extent and below the terrain: the same conditions."""
    sc, roots, q, _ = field_scenes(model)
    cam = VR.outside_camera(sc, float(roots[0, 1]))
    ref = VR.reference(sc, cam, VR.world_shapes(model, roots[:1], q[:1], np.float64), roots[:1, :3])
    rep = VR.render(sc, cam, VR.world_shapes(model, roots[:1], q[:1], np.float32), roots[:1, :3], dtype=np.float32)
    und = 1.0 - ref["decided"].mean()
    d = np.abs(rep["t"][0].astype(np.float64) - ref["ctr"]).max()
    fails = VR.failures(ref, rep["t"][0], rep["ids"][0], np.rint(rep["rgb"]), FIELD_SLACK)
    terrain = (ref["idset"][0] == 1).mean()
    print(f"outside and below: undecided {und:.2%}, terrain {terrain:.1%}, replay deviation {d:.3e} m "
          f"(held {FIELD_REPLAY_DEV:.3e}), failures {fails}")
    assert und <= UNDECIDED_CAP and terrain >= 0.3 and fails == (0, 0, 0)
    assert d <= FIELD_REPLAY_DEV


def test_scene_set_keeps_the_gpu_test_honest(model):
    """Per image: at most 2 % undecided pixels, robot and terrain both in view; the float32 replay of
    the reference passes the acceptance rule at every pixel and its centre deviation is the slack's
    source."""
    roots, q, scenes = scene_refs(model)
    sh32 = VR.world_shapes(model, roots, q, np.float32)
    plane = DR.scene(None)
    dev = 0.0
    for name, e, cam, sh, base in scenes:
        ref = VR.reference(plane, cam, sh, base)
        und = 1.0 - ref["decided"].mean()
        rep = VR.render(plane, cam, [sh32[e]], base, dtype=np.float32)
        d = np.abs(rep["t"][0].astype(np.float64) - ref["ctr"]).max()
        dev = max(dev, d)
        fails = VR.failures(ref, rep["t"][0], rep["ids"][0], np.rint(rep["rgb"]), SLACK)
        robot = (ref["idset"][0] >= 2).mean()
        print(f"{name}: undecided {und:.2%}, robot pixels {robot:.1%}, sky {(ref['idset'][0] == 0).mean():.1%}, "
              f"replay deviation {d:.3e} m, replay failures {fails}")
        assert und <= UNDECIDED_CAP, name
        assert robot >= 0.03, name
        assert fails == (0, 0, 0), name
    print(f"scene set: float32 replay centre deviation {dev:.3e} m (held {SCENE_REPLAY_DEV:.3e}, slack = 8 x)")
    assert dev <= SCENE_REPLAY_DEV
