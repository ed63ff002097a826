"""Stride statistics without a GPU: the sample function of csrc/hg_stride_sample.h (__host__
__device__, the code k_stride_sample runs) compiled for the host through tests/stride_host_shim.hip and
run over the planted sequences of tests/stride_cases.py against the float64 reference of
tests/stride_ref.py; the fold reference's bookkeeping; the config switch and the C ABI;
stride_report_row's arithmetic on hand-made accumulators.

Bounds: counts and every state slot exactly (the anchor, ref_hag and the max-built apex_hag are copies
or single differences of converted inputs); the float sums relative 1e-12 with absolute 1e-15
(metrics_ref.RTOL / ATOL, the project's bound for float sums of at most 100 steps: a sequence has 40
samples).  Inputs are float32 converted exactly, the arithmetic is double in a fixed order without
contraction, so the sample and the reference differ only by the rounding of sqrt and divide.
"""
import ctypes
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import metrics_ref as MR
import stride_cases as SC
import stride_ref as SR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "humanoid-gym-with-comments_amd", "csrc")
SHIM = os.path.join(REPO, "tests", "stride_host_shim.hip")
HEADER = os.path.join(CSRC, "hg_stride_sample.h")
f32 = np.float32


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _compile(out_dir, name, src=None):
    """The shim around `src` (default: the tree's header) as a shared object; nothing is launched."""
    so = os.path.join(str(out_dir), f"stride_host_{name}.so")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-O3", "-std=c++17", "-I", CSRC, SHIM, "-o", so]
    if src is not None:
        cmd.insert(1, f'-DHG_STRIDE_SRC="{src}"')
    subprocess.run(cmd, check=True, capture_output=True)
    L = ctypes.CDLL(so)
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    L.stride_sample_host.restype = ci
    L.stride_sample_host.argtypes = [ci, ci, vp, vp, vp, vp, vp, ci, ci, cf, cf, cf, ci, cd, vp, vp]
    L.stride_ground_host.restype = cd
    L.stride_ground_host.argtypes = [vp, ci, ci, cf, cf, cf, ci, cd, cd]
    return L


def _terrain_args(terrain):
    """(keep-alive array, hf pointer, rows, cols, hs, vs, border, terrain_type) for the shim."""
    if terrain is None:
        return None, None, 0, 0, 0.0, 0.0, 0.0, 0
    hf = np.ascontiguousarray(terrain["hf"], np.int16)
    return hf, hf.ctypes.data, hf.shape[0], hf.shape[1], float(terrain["hs"]), float(terrain["vs"]), float(terrain["border"]), 1


PAD_STATE, PAD_RUN = -7.25, 3.5    # what the padding columns hold: they must come back untouched


def host_sample(L, state, terrain, st, run, np_=None):
    """One sample of the host build on env-major `state`; st [16, n] / run [20, n] are copied into
    padded SoA buffers (row stride np_), updated, and returned whole (padding columns as well)."""
    n = state["root_states"].shape[0]
    np_ = np_ or (n + 63) // 64 * 64
    soa = SC.to_soa(state, np_)
    s = np.full((2 * SR.NST, np_), PAD_STATE, np.float64)
    r = np.full((2 * SR.NS, np_), PAD_RUN, np.float64)
    s[:, :n], r[:, :n] = st, run
    feet = np.asarray(SC.FEET, np.int32)
    keep, *targs = _terrain_args(terrain)
    p = lambda a: a.ctypes.data  # noqa: E731
    taken = L.stride_sample_host(n, np_, p(soa["root_states"]), p(soa["contact_forces"]), p(soa["rigid_state"]), p(feet),
                                 *targs, SC.DT, p(s), p(r))
    del keep
    return s, r, taken


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    return _compile(tmp_path_factory.mktemp("stride_host"), "tree")


@pytest.fixture(scope="module")
def ref_runs():
    """The reference's final (state, run, ok) of both groups, computed once."""
    return {key: SR.replay(SC.group(key)[1], SC.TERRAINS[key], SC.DT) for key in SC.TERRAINS}


def _col(ref_runs, key, name):
    names = SC.group(key)[0]
    st, run, ok = ref_runs[key]
    e = names.index(name)
    return st[:, e], run[:, e], ok[:, e]


# ---------------------------------------------------------------- the cases' promises
def test_cases_keep_their_promises(ref_runs):
    """The sequences do what their names say, by hand-derivable values of the reference's own sums."""
    g = lambda run, f, k: float(run[f * SR.NS + SR.NAMES.index(k)])  # noqa: E731
    s = lambda st, f, k: float(st[f * SR.NST + SR.STATE_NAMES.index(k)])  # noqa: E731
    assert all(c[1]["root_states"].shape[0] <= 40 for c in SC.CASES)
    # clean walk: one swing of 26 samples, 10 cm high, 0.3 m wide; the other foot lifts off at the end
    st, run, ok = _col(ref_runs, "plane", "clean_walk")
    assert ok.all() and g(run, 0, "strides") == 1 and g(run, 0, "swing_time") == 26 * SC.DT
    assert 0.099 < g(run, 0, "clearance") < 0.1 and abs(g(run, 0, "step_width") - 0.3) < 1e-6
    assert abs(g(run, 0, "step_length") - 26 * 2 * 0.6 * SC.DT) < 1e-6 and g(run, 0, "stride_pairs") == 0
    assert g(run, 0, "touchdown_force") == SC.FORCE + 32 and not run[SR.NS:].any()
    assert (s(st, 1, "phase"), s(st, 1, "phase_steps")) == (2, 2) and (s(st, 0, "phase"), s(st, 0, "phase_steps")) == (1, 8)
    # quick walk: two touchdowns per foot 16 samples apart: one stride pair each
    st, run, _ = _col(ref_runs, "plane", "quick_walk")
    for f in range(2):
        assert g(run, f, "strides") == 2 and g(run, f, "stride_pairs") == 1 and g(run, f, "stride_time") == 16 * SC.DT
        assert abs(g(run, f, "stride_length") - 6 * 2 * 0.6 * SC.DT) < 1e-6 and g(run, f, "short_swings") == 0
    # the episode opens mid-swing: the first touchdown anchors and counts nothing, the second is a stride with a pair
    st, run, _ = _col(ref_runs, "plane", "opens_mid_swing")
    assert g(run, 0, "strides") == 1 and g(run, 0, "stride_pairs") == 1 and g(run, 0, "stride_time") == 20 * SC.DT
    assert g(run, 0, "swing_time") == 8 * SC.DT
    # swings of 1, 2 and 3 samples: two are chatter, the third counts; chatter leaves the anchor alone
    st, run, _ = _col(ref_runs, "plane", "swing_1_2_3")
    for f in range(2):
        assert g(run, f, "short_swings") == 2 and g(run, f, "strides") == 1 and g(run, f, "swing_time") == 3 * SC.DT
    assert g(run, 1, "stride_pairs") == 0 and s(st, 1, "since_td") == 39 - 6       # anchored at t = 6 by the 3-sample swing
    # exactly 5.0 is no contact, the next float32 is: a 10-sample swing that lands with a force just above 5
    _, run, _ = _col(ref_runs, "plane", "force_5_and_next")
    assert g(run, 0, "strides") == 1 and g(run, 0, "swing_time") == 10 * SC.DT
    assert 5.0 < g(run, 0, "touchdown_force") < 5.000001
    # heading: the same walk turned, rolled and pitched, or with a scaled quaternion keeps its step figures
    _, ref, _ = _col(ref_runs, "plane", "quick_walk")
    for name in ("yaw_90", "yaw_180", "rolled_pitched", "quat_scaled_3p7", "far_180m"):
        _, run, ok = _col(ref_runs, "plane", name)
        tol = 1e-4 if name == "far_180m" else 1e-6          # float32 positions 180 m out: 1.5e-5 apart
        assert ok.all()
        for f in range(2):
            for k in ("step_length", "step_width", "stride_length"):
                assert abs(g(run, f, k) - g(ref, f, k)) < tol, (name, f, k)
            assert g(run, f, "strides") == 2
    _, a, _ = _col(ref_runs, "plane", "rolled_pitched")
    _, b, _ = _col(ref_runs, "plane", "quat_scaled_3p7")
    assert np.allclose(a, b, rtol=0, atol=1e-6)
    # a zero quaternion has no heading: every sample counts as non-finite
    st, run, ok = _col(ref_runs, "plane", "quat_zero")
    assert not ok.any() and not run.any() and not st.any()
    # both feet land on one sample (t = 11 and t = 28); flight: both feet in the air at once
    for name in ("both_land_together", "flight"):
        st, run, _ = _col(ref_runs, "plane", name)
        assert [g(run, f, "strides") for f in range(2)] == [2, 2] and s(st, 0, "since_td") == s(st, 1, "since_td") == 11
    assert g(_col(ref_runs, "plane", "both_land_together")[1], 0, "step_length") > 0.03
    # the foot only descends: the clearance is negative
    _, run, _ = _col(ref_runs, "plane", "foot_only_descends")
    assert g(run, 0, "strides") == 1 and -0.01 < g(run, 0, "clearance") < 0
    # non-finite mid-swing: one sample is skipped, the interrupted swing is no stride and no pair crosses the gap
    _, whole, _ = _col(ref_runs, "plane", "nan_where_not_read")
    assert [g(whole, f, "strides") for f in range(2)] == [2, 2] and [g(whole, f, "stride_pairs") for f in range(2)] == [1, 1]
    for name in SC.NAMES:
        if name.startswith(("nan_", "inf_", "neg_inf_")) and name != "nan_where_not_read":
            st, run, ok = _col(ref_runs, "plane", name)
            assert (~ok).sum() == 1, name
            assert [g(run, f, "strides") for f in range(2)] == [1, 2] and not g(run, 0, "stride_pairs") and not g(run, 1, "stride_pairs")
            assert s(st, 0, "has_anchor") == 1        # re-anchored by the touchdown of the swing whose lift-off was lost
    assert {"nan_root_quat", "inf_contact_z", "nan_rigid_pos"} <= set(SC.NAMES)      # each read array in turn
    # the heightfield: on the field a foot that follows the step up keeps a 10 cm clearance, on the plane the
    # same sequence reads the step's height as clearance; stepping down, the plane run is negative
    _, on_field, _ = _col(ref_runs, "field", "field_crosses_edge")
    _, on_plane, _ = _col(ref_runs, "plane", "field_crosses_edge")
    assert abs(g(on_field, 0, "clearance") / 2 - 0.0985) < 1e-3 and g(on_plane, 0, "clearance") > g(on_field, 0, "clearance") + 0.08
    assert g(_col(ref_runs, "plane", "field_descends_edge")[1], 0, "clearance") < -0.1
    assert 0 < g(_col(ref_runs, "field", "field_descends_edge")[1], 0, "clearance") < 0.03
    st, _, _ = _col(ref_runs, "field", "field_outside_clamped")
    assert abs(s(st, 0, "ref_hag") - (SC.ANKLE - 0.2)) < 1e-6          # clamped to the last cell: the step's 40 * 0.005
    # the notch: at cell (3, 3) the minimum of three neighbours is the neighbour's 30, not the own 40
    assert SR.ground(0.3, 0.3, SC.FIELD) == float(f32(0.005)) * 30 and SR.ground(0.3, -0.3, SC.FIELD) == float(f32(0.005)) * 40
    assert SR.ground(0.1, 0.1, SC.FIELD) == 0 and SR.ground(-9.0, 0.1, SC.FIELD) == 0 and SR.ground(0.3, 0.3, None) == 0


# ---------------------------------------------------------------- the host sample on every sequence
@pytest.mark.parametrize("key", ["plane", "field"])
def test_host_sample_on_every_sequence(host, key):
    """Every sample of every sequence, compared after each one: state and counts exactly, sums within
    the bound; the padding columns keep their bits; a skipped sample is reported."""
    names, seq = SC.group(key)
    n = len(names)
    terrain = SC.TERRAINS[key]
    st_ref, run_ref = np.zeros((2 * SR.NST, n)), np.zeros((2 * SR.NS, n))
    st_got, run_got = st_ref.copy(), run_ref.copy()
    worst = 0.0
    for t in range(SC.T):
        state = {k: seq[k][t] for k in SR.STATE_KEYS}
        st_ref, run_ref, ok = SR.sample(state, terrain, SC.DT, st_ref, run_ref)
        s, r, taken = host_sample(host, state, terrain, st_got, run_got)
        assert taken == ok.sum()
        assert (s[:, n:] == PAD_STATE).all() and (r[:, n:] == PAD_RUN).all()     # columns e >= n are never written
        st_got, run_got = s[:, :n], r[:, :n]
        worst = max(worst, SR.compare(st_got, run_got, st_ref, run_ref))
        np.testing.assert_array_equal(st_got[SR.STATE_NAMES.index("apex_hag")], st_ref[SR.STATE_NAMES.index("apex_hag")])
    for e, name in enumerate(names):
        print(f"{key:6s} {name:26s} strides {run_got[0, e]:.0f}/{run_got[SR.NS, e]:.0f} "
              f"clearance {run_got[2, e]:+.4f}/{run_got[SR.NS + 2, e]:+.4f}")
    print(f"host sample on the {key}: largest deviation {worst:.3e} x the bound (rtol {MR.RTOL}, atol {MR.ATOL})")
    assert worst <= 1.0
    assert np.isfinite(run_got).all() and np.isfinite(st_got).all()
    assert run_got[0].sum() + run_got[SR.NS].sum() >= n        # the group as a whole counts strides


def test_host_ground_rule(host):
    """hg_stride_ground against the reference on a grid of points over and around the field, cell
    borders included, and on the plane."""
    keep, *targs = _terrain_args(SC.FIELD)
    pts = [f32(v) for v in np.concatenate([np.linspace(-1.0, 1.25, 37), [-0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1e6, -1e6, 3e38]])]
    for x in pts:
        for y in pts:
            assert host.stride_ground_host(*targs, float(x), float(y)) == SR.ground(x, y, SC.FIELD), (x, y)
    assert host.stride_ground_host(None, 0, 0, 0.0, 0.0, 0.0, 0, 0.3, 0.3) == 0.0
    assert host.stride_ground_host(*targs[:-1], 0, 0.3, 0.3) == 0.0          # terrain_type 0 wins over a field pointer
    del keep


# ---------------------------------------------------------------- wrong samples
# (name, the text replaced, its replacement, sequences that must fail)
WRONG = [
    ("contact_ge", "const bool contact = fz[f] > HG_METRICS_CONTACT_Z;", "const bool contact = fz[f] >= HG_METRICS_CONTACT_Z;",
     ["force_5_and_next"]),
    ("chatter_counts", "if (steps < (double)HG_STRIDE_MIN_SWING) {", "if (steps < 2.0) {", ["swing_1_2_3"]),
    ("quat_not_normalised", "const double qn = 1.0 / sqrt(", "const double qn = 1.0 + 0.0 * sqrt(", ["quat_scaled_3p7"]),
    ("lateral_sign_lost", "lat = ry * hx - rx * hy;", "lat = ry * hx + rx * hy;", ["rolled_pitched", "far_180m"]),
    ("ref_follows_the_swing", "} else if (!contact) {  // swing goes on", "} else if (s[HG_SS_REF_HAG * st] = hag[f], !contact) {",
     ["clean_walk", "quick_walk"]),
    ("clearance_never_negative", "r[HG_SD_CLEARANCE * st] += s[HG_SS_APEX_HAG * st] - s[HG_SS_REF_HAG * st];",
     "r[HG_SD_CLEARANCE * st] += fmax(0.0, s[HG_SS_APEX_HAG * st] - s[HG_SS_REF_HAG * st]);", ["foot_only_descends"]),
    ("mid_swing_opening_counts", "const int phase = (int)s[HG_SS_PHASE * st];",
     "const int phase = (int)s[HG_SS_PHASE * st] == 3 ? 2 : (int)s[HG_SS_PHASE * st];", ["opens_mid_swing"]),
    ("own_cell_only", "h = h1 < h ? h1 : h;", "h = h1 < h ? h : h;", ["field_crosses_edge"]),
    ("float_arithmetic", "const double along = rx * hx + ry * hy,", "const double along = (float)(rx * hx + ry * hy),",
     ["rolled_pitched", "far_180m"]),
    ("gap_keeps_the_state", "for (int k = 0; k < 2 * HG_STRIDE_STATE_SLOTS; k++) s0[k * st] = 0.0;", ";", ["nan_root_quat", "inf_contact_z"]),
]


@pytest.fixture(scope="module")
def wrong(tmp_path_factory, host):
    out = tmp_path_factory.mktemp("stride_wrong")
    text = open(HEADER).read()
    jobs = []
    for name, old, new, _ in WRONG:
        assert text.count(old) == 1, f"{name}: the replaced text matches {text.count(old)} times"
        src = os.path.join(str(out), f"hg_stride_sample_{name}.h")
        with open(src, "w") as f:
            f.write(text.replace(old, new))
        jobs.append((name, src))
    with ThreadPoolExecutor(3) as ex:
        libs = list(ex.map(lambda j: _compile(out, j[0], j[1]), jobs))
    return {name: L for (name, _), L in zip(jobs, libs)}


def _failing_cases(L, key, ref):
    names, seq = SC.group(key)
    n = len(names)
    st, run = np.zeros((2 * SR.NST, n)), np.zeros((2 * SR.NS, n))
    for t in range(SC.T):
        s, r, _ = host_sample(L, {k: seq[k][t] for k in SR.STATE_KEYS}, SC.TERRAINS[key], st, run)
        st, run = s[:, :n], r[:, :n]
    bad = []
    for e, name in enumerate(names):
        try:
            dev = SR.compare(st[:, e], run[:, e], ref[0][:, e], ref[1][:, e])
        except AssertionError:
            dev = np.inf
        if dev > 1.0:
            bad.append(name)
    return bad


@pytest.mark.parametrize("name", [w[0] for w in WRONG])
def test_wrong_sample_fails_the_cases(wrong, ref_runs, name):
    """The sequences see a one-line mistake: the named ones leave the bound."""
    expect = next(w[3] for w in WRONG if w[0] == name)
    key = "field" if any(e.startswith("field_") for e in expect) else "plane"
    bad = _failing_cases(wrong[name], key, ref_runs[key])
    print(f"{name}: fails {bad}")
    assert set(expect) <= set(bad), f"{name}: passes {sorted(set(expect) - set(bad))}"


# ---------------------------------------------------------------- fold rules
def test_fold_reference_bookkeeping():
    """The fold statement the GPU tests compare with, on a hand-made case: env 0 resets mid-swing, env
    1 resets in stance, env 2 runs on mid-swing, env 3 runs on."""
    n = 4
    st = np.zeros((2 * SR.NST, n))
    run = np.arange(1, 2 * SR.NS * n + 1, dtype=np.float64).reshape(2 * SR.NS, n)
    done = np.full((2 * SR.NS, n), 100.0)
    st[0] = (2, 1, 2, 1)            # foot 0: envs 0 and 2 swing
    st[1] = (5, 9, 7, 3)
    st[SR.NST + 0] = 1
    st[SR.NST + 4] = (0.5, 0.25, 0.125, 2.0)
    s, r, d = SR.fold(st, run, done, 0, reset=[1, 1, 0, 0])
    assert not s[:, :2].any() and not r[:, :2].any()                     # the swing in progress is discarded
    assert np.array_equal(d[:, :2], 100.0 + run[:, :2]) and np.array_equal(d[:, 2:], done[:, 2:])
    assert np.array_equal(s[:, 2:], st[:, 2:]) and np.array_equal(r[:, 2:], run[:, 2:])
    s, r, d = SR.fold(st, run, done, 1, mask=[0, 1, 0, 1])
    assert np.array_equal(d, done)                                       # a discard adds nothing
    assert not s[:, [1, 3]].any() and not r[:, [1, 3]].any()
    assert np.array_equal(s[:, [0, 2]], st[:, [0, 2]]) and np.array_equal(r[:, [0, 2]], run[:, [0, 2]])
    s, r, d = SR.fold(st, run, done, 1)                                  # the NULL mask: every env
    assert not s.any() and not r.any() and np.array_equal(d, done)
    # a stride interrupted by a reset is no stride: the next episode opens mid-swing and only anchors
    names, seq = SC.group("plane")
    e = names.index("clean_walk")
    one = {k: seq[k][:, e:e + 1] for k in SR.STATE_KEYS}
    s, r = np.zeros((2 * SR.NST, 1)), np.zeros((2 * SR.NS, 1))
    d = np.zeros_like(r)
    for t in range(SC.T):
        s, r, _ = SR.sample({k: one[k][t] for k in SR.STATE_KEYS}, None, SC.DT, s, r)
        s, r, d = SR.fold(s, r, d, 0, reset=[t == 20])
    assert not d.any() and not r[:SR.NS].any() and s[SR.STATE_NAMES.index("has_anchor"), 0] == 1


# ---------------------------------------------------------------- config and ABI
def test_switch_is_off_by_default_and_needs_the_gait_metrics():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    assert cfg.metrics.strides is False
    _, js = N.load_model()
    cfg.metrics.gait = True
    assert build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)[0].gait_metrics == 1
    cfg.metrics.strides = True
    assert build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)[0].gait_metrics == 3
    cfg.metrics.gait = False
    with pytest.raises(ValueError, match="metrics.strides needs metrics.gait"):
        build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert N.STRIDE_NAMES == SR.NAMES and N.STRIDE_STATE_NAMES == SR.STATE_NAMES
    from humanoid.scripts import evaluate as EV
    assert EV.make_cfg(16, 5.0).metrics.strides is False
    on = EV.make_cfg(16, 5.0, strides=True)
    assert on.metrics.strides is True and on.metrics.gait is True


def test_header_table_ids_and_source_stamp(tmp_path):
    from humanoid import _native as N
    src = open(os.path.join(REPO, "include", "hgsim.h")).read()
    for k, name in enumerate(SR.NAMES):                 # the header documents every slot, in order
        assert re.search(r"stride\s+%d\s+%s\b" % (k, name), src), name
    for k, name in enumerate(SR.STATE_NAMES):
        assert re.search(r"state\s+%d\s+%s\b" % (k, name), src), name
    ids = ["METRICS_COUNT", "STRIDE_RUN", "STRIDE_DONE", "STRIDE_STATE"]
    assert [N.T[k] - N.T[ids[0]] for k in ids] == [0, 1, 2, 3]         # directly after the metrics ids
    c = tmp_path / "ids.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hgsim.h"\nint main(){printf("%d %d %d %d %d %zu %zu",'
                 'HG_T_METRICS_COUNT,HG_T_STRIDE_RUN,HG_T_STRIDE_DONE,HG_T_STRIDE_STATE,HG_T_COUNT,'
                 'offsetof(hg_cfg,gait_metrics),sizeof(hg_cfg));}')
    exe = tmp_path / "ids"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [N.T[k] for k in ids] + [len(N.TENSOR_IDS), N.HgCfg.gait_metrics.offset, ctypes.sizeof(N.HgCfg)]
    # the header's constants are the names' lengths
    hdr = open(HEADER).read()
    assert re.search(r"#define HG_STRIDE_SLOTS %d\b" % SR.NS, hdr) and re.search(r"#define HG_STRIDE_STATE_SLOTS %d\b" % SR.NST, hdr)
    assert re.search(r"#define HG_STRIDE_MIN_SWING %d\b" % SR.MIN_SWING, hdr)
    # the build stamps the new files: the Makefile's list and source_hash's are the same, in the same order
    mk = open(os.path.join(REPO, "humanoid-gym-with-comments_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    stamp = re.search(r"^STAMP_SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "csrc/hg_stride.hip" in srcs and "csrc/hg_stride_sample.h" in stamp
    import hashlib
    h = hashlib.sha256()
    for rel in srcs + stamp[1:]:
        with open(os.path.join(REPO, "humanoid-gym-with-comments_amd", rel), "rb") as f:
            h.update(f.read())
    assert N.source_hash() == h.hexdigest()[:16]


def test_library_refuses_and_sizes_without_a_gpu():
    """No GPU needed: gait_metrics = 2 (strides without the metrics) is refused with a reason, a NULL
    sim is refused by name, and the arena grows by the three stride buffers only with bit 1."""
    from humanoid import _native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    L = N.load_library()
    for fn, args in (("hg_metrics_sample", (None, None)), ("hg_metrics_fold", (None, 0, None, None)),
                     ("hg_metrics_clear", (None, None))):
        assert getattr(L, fn)(*args) == 1 and (fn + ": sim is NULL").encode() in L.hg_last_error(None)
    c = N.HgCfg()
    c.num_envs, c.frame_stack, c.c_frame_stack = 65, 15, 3
    base = L.hg_arena_bytes(ctypes.byref(c))
    c.gait_metrics = 1
    one = L.hg_arena_bytes(ctypes.byref(c))
    assert one - base == 2 * 13 * 128 * 8 + 4 * 128 * 4          # what gait_metrics = 1 has always added
    c.gait_metrics = 3
    assert L.hg_arena_bytes(ctypes.byref(c)) - one == 2 * 20 * 128 * 8 + 16 * 128 * 8
    # hg_create checks the field before it touches the arena: a model of the right shape, everything else valid
    m, js = N.load_model()
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    sim = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(512)
    arena = ctypes.c_void_p((ctypes.addressof(buf) + 255) & ~255)
    for bad in (2, 4, -1):
        hc.gait_metrics = bad
        assert L.hg_create(ctypes.byref(hc), ctypes.byref(m), arena, 1 << 40, ctypes.byref(sim)) == 1
        assert b"gait_metrics" in L.hg_last_error(None) and b"strides" in L.hg_last_error(None), L.hg_last_error(None)
        assert not sim.value


# ---------------------------------------------------------------- stride_report_row's arithmetic
def _accumulators():
    """Two envs: env 0 has 2 episodes, env 1 has 1; left and right differ."""
    i = SR.NAMES.index
    done = np.zeros((2 * SR.NS, 2))
    counts = np.zeros((4, 2), np.int64)
    counts[0] = (2, 1)
    L, R = 0, SR.NS
    done[L + i("strides")] = (6, 4)
    done[L + i("swing_time")] = (1.5, 1.0)
    done[L + i("clearance")] = (0.6, 0.2)
    done[L + i("step_length")] = (2.0, 1.0)
    done[L + i("step_width")] = (1.5, 1.5)
    done[L + i("touchdown_force")] = (3000.0, 2000.0)
    done[L + i("stride_pairs")] = (5, 3)
    done[L + i("stride_length")] = (4.0, 2.0)
    done[L + i("stride_time")] = (3.0, 2.0)
    done[L + i("short_swings")] = (1, 1)
    done[R + i("strides")] = (5, 3)
    done[R + i("swing_time")] = (1.0, 1.0)
    done[R + i("clearance")] = (0.5, 0.5)
    done[R + i("step_length")] = (1.0, 1.0)
    done[R + i("step_width")] = (1.0, 1.0)
    done[R + i("touchdown_force")] = (2400.0, 1600.0)
    done[R + i("stride_pairs")] = (4, 0)
    done[R + i("stride_length")] = (3.0, 0.0)
    done[R + i("stride_time")] = (2.0, 0.0)
    return done, counts


def test_stride_report_on_hand_made_accumulators():
    from humanoid.envs.custom.humanoid_env import stride_report_arrays, stride_report_row
    done, counts = _accumulators()
    rep = stride_report_row(done, counts, 0.01, 0.1, 0.64)
    assert sorted(rep) == ["both", "left", "right"]
    le, ri, bo = rep["left"], rep["right"], rep["both"]
    assert (le["strides"], ri["strides"], bo["strides"]) == (10, 8, 18)
    assert le["strides_per_episode"] == 10 / 3 and bo["strides_per_episode"] == 6.0
    assert le["mean_swing_time"] == 0.25 and ri["mean_swing_time"] == 0.25 and bo["mean_swing_time"] == 4.5 / 18
    assert le["mean_clearance"] == 0.8 / 10 and le["clearance_vs_target"] == (0.8 / 10) / 0.1
    assert ri["mean_clearance"] == 0.125 and ri["clearance_vs_target"] == 0.125 / 0.1
    assert le["mean_step_length"] == 0.3 and ri["mean_step_length"] == 0.25 and le["mean_step_width"] == 0.3
    assert le["mean_touchdown_force"] == 500.0 and ri["mean_touchdown_force"] == 500.0 and bo["mean_touchdown_force"] == 500.0
    assert le["mean_stride_length"] == 0.75 and ri["mean_stride_length"] == 0.75
    assert le["mean_stride_time"] == 0.625 and ri["mean_stride_time"] == 0.5 and bo["mean_stride_time"] == 7.0 / 12
    assert le["stride_time_vs_cycle"] == 0.625 / 0.64
    assert le["cadence"] == 1 / 0.625 and ri["cadence"] == 2.0 and bo["cadence"] == 2 / (7.0 / 12)
    assert le["swing_fraction"] == 0.25 / 0.625 and ri["swing_fraction"] == 0.5
    assert le["short_swing_fraction"] == 2 / 12 and ri["short_swing_fraction"] == 0.0
    assert bo["swing_time_asymmetry"] == 0.0
    assert bo["step_length_asymmetry"] == (0.3 - 0.25) / ((0.3 + 0.25) / 2.0)
    assert "swing_time_asymmetry" not in le and "step_length_asymmetry" not in ri
    assert set(bo) - set(le) == {"swing_time_asymmetry", "step_length_asymmetry"}
    # per terrain type: env 0 is type 2, env 1 type 5; env 1's right foot has no stride pair
    by = stride_report_arrays(done, counts, 0.01, 0.1, 0.64, terrain_types=[2, 5])
    assert by["overall"] == rep and sorted(by["terrain_types"]) == [2, 5]
    t5 = by["terrain_types"][5]
    assert t5["right"]["mean_stride_time"] is None and t5["right"]["cadence"] is None and t5["right"]["swing_fraction"] is None
    assert t5["right"]["stride_time_vs_cycle"] is None and t5["right"]["mean_stride_length"] is None
    assert t5["left"]["strides_per_episode"] == 4.0 and t5["both"]["mean_stride_time"] == 2.0 / 3


def test_stride_report_with_zero_divisors_gives_none():
    from humanoid.envs.custom.humanoid_env import stride_report_row
    rep = stride_report_row(np.zeros((2 * SR.NS, 3)), np.zeros((4, 3), np.int64), 0.01, 0.1, 0.64)
    for side in ("left", "right", "both"):
        assert rep[side]["strides"] == 0
        for k, v in rep[side].items():
            assert k == "strides" or v is None, (side, k, v)
    # a target or a cycle time of zero: the comparison is None, the mean is a number
    done, counts = _accumulators()
    rep = stride_report_row(done, counts, 0.01, 0.0, 0.0)
    assert rep["left"]["clearance_vs_target"] is None and rep["left"]["stride_time_vs_cycle"] is None
    assert rep["left"]["mean_clearance"] == 0.08
    # equal and opposite step lengths: the asymmetry's divisor is zero
    i = SR.NAMES.index
    done[SR.NS + i("step_length")] = (-1.2, -1.2)              # 8 strides: the mean is -0.3 against the left foot's 0.3
    rep = stride_report_row(done, counts, 0.01, 0.1, 0.64)
    assert rep["left"]["mean_step_length"] == -rep["right"]["mean_step_length"] and rep["both"]["step_length_asymmetry"] is None


def test_evaluate_formats_the_stride_report():
    from humanoid.envs.custom.humanoid_env import stride_report_arrays
    from humanoid.scripts import evaluate as EV
    done, counts = _accumulators()
    rep = stride_report_arrays(done, counts, 0.01, 0.1, 0.64, terrain_types=[2, 5])
    lines = EV.format_stride_report(rep).splitlines()
    assert lines[0].split() == ["overall", "left", "right", "both"]
    assert len(lines) == 3 * (1 + len(EV.STRIDE_ROW_ORDER))               # overall and two terrain types
    assert set(EV.STRIDE_ROW_ORDER) == set(rep["overall"]["both"])
    row = {ln.split()[0]: ln.split()[1:] for ln in lines[1:1 + len(EV.STRIDE_ROW_ORDER)]}
    assert row["strides"] == ["10", "8", "18"] and row["mean_swing_time"] == ["0.2500", "0.2500", "0.2500"]
    assert row["swing_time_asymmetry"] == ["0.0000"]                     # only the `both` column has it
    one = stride_report_arrays(done, counts, 0.01, 0.1, 0.64, terrain_types=[0, 0])
    assert len(EV.format_stride_report(one).splitlines()) == 1 + len(EV.STRIDE_ROW_ORDER)
