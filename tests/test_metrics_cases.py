"""Gait metrics without a GPU: the sample function of csrc/hg_metrics_sample.h (__host__ __device__,
the code k_metrics_sample runs) compiled for the host through tests/metrics_host_shim.hip and run
over the planted rows of tests/metrics_cases.py against the float64 reference of tests/metrics_ref.py;
the fold reference's bookkeeping; the config switch and the C ABI; gait_report's arithmetic on
hand-made accumulators.

Bound on the float sums: relative 1e-12 with absolute 1e-15 (metrics_ref.RTOL / ATOL).  Inputs are
float32 converted exactly, the arithmetic is double in a fixed order without contraction, so the
sample and the reference differ only by the rounding of sqrt and divide: a few roundings per sample.
"""
import ctypes
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import metrics_cases as MC
import metrics_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "humanoid-gym-with-comments_amd", "csrc")
SHIM = os.path.join(REPO, "tests", "metrics_host_shim.hip")
HEADER = os.path.join(CSRC, "hg_metrics_sample.h")
f32 = np.float32


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def _compile(out_dir, name, src=None):
    """The shim around `src` (default: the tree's header) as a shared object; nothing is launched."""
    so = os.path.join(str(out_dir), f"metrics_host_{name}.so")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-O3", "-std=c++17", "-I", CSRC, SHIM, "-o", so]
    if src is not None:
        cmd.insert(1, f'-DHG_METRICS_SRC="{src}"')
    subprocess.run(cmd, check=True, capture_output=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.metrics_sample_host.restype = ctypes.c_int
    L.metrics_sample_host.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 10 + [ctypes.c_double, vp, vp]
    return L


def host_sample(L, state, run, counts, np_=None):
    """One sample of the host build on env-major `state`; run [13, n] / counts [4, n] are copied into
    padded SoA buffers (row stride np_), updated, and returned with the padding columns as well."""
    n = state["root_states"].shape[0]
    np_ = np_ or (n + 63) // 64 * 64
    soa = MC.to_soa(state, np_)
    r = np.zeros((13, np_), np.float64)
    c = np.zeros((4, np_), np.int32)
    r[:, :n], c[:, :n] = run, counts
    feet = np.asarray(MC.FEET, np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731
    added = L.metrics_sample_host(n, np_, *[p(soa[k]) for k in MR.STATE_KEYS], p(feet), p(MC.TORQUE_LIMIT), MC.DT, p(r), p(c))
    return r, c, added


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip("no hipcc")
    return _compile(tmp_path_factory.mktemp("metrics_host"), "tree")


def _prior(n, seed=3):
    """A running row that already holds an episode's worth of sums (so += and max are both visible);
    the peak of every third env is above anything a row produces."""
    rs = np.random.RandomState(seed)
    run = rs.uniform(0.0, 3.0, (13, n))
    run[0] = rs.randint(1, 50, n)
    run[12] = np.where(np.arange(n) % 3 == 0, 7.5, 0.01)
    counts = rs.randint(0, 5, (4, n))
    return run, counts


# ---------------------------------------------------------------- the table's promises
def test_table_keeps_its_promises():
    """The rows do what their names say, by hand-derivable values of the reference's own terms."""
    T, ok = MR.sample_terms(MC.stack(range(len(MC.ROWS))), MC.TORQUE_LIMIT, MC.DT)
    t = {n: T[:, i] for i, n in enumerate(MC.NAMES)}
    slot = MR.NAMES.index
    assert len(set(MC.NAMES)) == len(MC.NAMES)
    assert [not o for o in ok] == MC.SKIPPED and sum(MC.SKIPPED) == 10
    for k in MR.STATE_KEYS:                      # a NaN in each input array in turn
        assert "nan_" + k in MC.NAMES
    # the scaled quaternion is the walking row's rotation: the same frame terms up to rounding
    q0, q1 = MC.ROWS[0][1]["root_states"][3:7].astype(np.float64), MC.ROWS[1][1]["root_states"][3:7].astype(np.float64)
    assert abs(np.linalg.norm(q1) - 3.7) < 1e-6 and np.allclose(q1 / 3.7, q0, atol=1e-7)
    # rolled 90 degrees: gravity lies along the base y axis, tilt2 = 1; v_b.y is the world -z... of a rolled base
    assert abs(t["rolled_90"][slot("tilt2")] - 1.0) < 1e-7
    r = MC.ROWS[2][1]
    vb_y = float(r["root_states"][9])            # base y axis = world z after a +90 degree roll about x
    assert abs(t["rolled_90"][slot("err_vy2")] - (vb_y - float(r["commands"][1])) ** 2) < 1e-7
    # mixed power: the clamp is per joint (positive products only), not on the sum
    m = MC.ROWS[MC.NAMES.index("mixed_power")][1]
    p = m["torques"].astype(np.float64) * m["dof_vel"].astype(np.float64)
    assert (p < 0).sum() >= 3 and (p > 0).sum() >= 3
    assert t["mixed_power"][slot("work_pos")] == p[p > 0].sum() * MC.DT != max(p.sum(), 0.0) * MC.DT
    # exactly 5.0 is no contact, the next float32 is: one foot down, its slip alone
    fr = MC.ROWS[MC.NAMES.index("force_5_and_next")][1]
    assert fr["contact_forces"][MC.FEET[0], 2] == f32(5.0) < fr["contact_forces"][MC.FEET[1], 2] < f32(5.000001)
    assert t["force_5_and_next"][slot("double_support")] == 0 and t["force_5_and_next"][slot("flight")] == 0
    v = fr["rigid_state"][MC.FEET[1], 7:9].astype(np.float64)
    assert t["force_5_and_next"][slot("slip")] == np.sqrt(v[0] * v[0] + v[1] * v[1]) * MC.DT
    # a torque exactly at its limit: ratio exactly 1, the others 0.5
    assert t["torque_at_limit"][slot("peak_torque")] == 1.0
    # all-zero velocities: no distance, work or slip; tracking error is the command itself
    z = t["zero_velocities"]
    assert z[slot("distance")] == 0 and z[slot("work_pos")] == 0 and z[slot("slip")] == 0
    assert z[slot("err_vx2")] == float(MC.ROWS[MC.NAMES.index("zero_velocities")][1]["commands"][0]) ** 2
    assert t["double_support"][slot("double_support")] == 1 and t["flight"][slot("flight")] == 1
    assert t["walking"][slot("double_support")] == 0 and t["walking"][slot("flight")] == 0
    assert ok[MC.NAMES.index("nan_where_not_read")]


# ---------------------------------------------------------------- the host sample on the table
def test_host_sample_on_every_row(host):
    """Two samples on top of a prior running row; in the second every env sees the next row of the
    table.  Skipped rows keep their bits and count one skip each time."""
    n = len(MC.ROWS)
    run0, cnt0 = _prior(n)
    worst = 0.0
    run_ref, cnt_ref = run0, cnt0
    run_got, cnt_got = run0, cnt0
    for rnd in range(2):
        idx = [(i + rnd) % n for i in range(n)]
        st = MC.stack(idx)
        before = run_got.copy()
        run_ref, cnt_ref = MR.sample(st, MC.TORQUE_LIMIT, MC.DT, run_ref, cnt_ref)
        r, c, added = host_sample(host, st, run_got, cnt_got)
        run_got, cnt_got = r[:, :n], c[:, :n]
        assert not r[:, n:].any() and not c[:, n:].any()          # the padding columns are never written
        skipped = np.array([MC.SKIPPED[i] for i in idx])
        assert added == n - skipped.sum()
        assert np.isfinite(run_got).all()
        assert np.array_equal(run_got[:, skipped], before[:, skipped])   # unchanged, bit for bit
        np.testing.assert_array_equal(cnt_got, cnt_ref)
        for e in range(n):
            dev = MR.max_deviation(run_got[:, e], run_ref[:, e])
            worst = max(worst, dev)
            print(f"round {rnd} env {e:2d} {MC.NAMES[idx[e]]:24s} deviation {dev * MR.RTOL:.2e} relative")
        # integer-valued slots and the running max are exact
        for s in ("steps", "double_support", "flight"):
            np.testing.assert_array_equal(run_got[MR.NAMES.index(s)], run_ref[MR.NAMES.index(s)])
    print(f"host sample: largest deviation {worst:.3e} x the bound (rtol {MR.RTOL}, atol {MR.ATOL})")
    assert worst <= 1.0
    assert (cnt_got[3] - cnt0[3]).sum() == 2 * sum(MC.SKIPPED)
    # the prior peak survives where it is the larger one, and is replaced where it is not
    pk = MR.NAMES.index("peak_torque")
    assert (run_got[pk] == 7.5).sum() == (n + 2) // 3 and (run_got[pk] > 0.01).sum() >= n // 2
    np.testing.assert_array_equal(run_got[pk], run_ref[pk])      # a max is exact


def test_fold_reference_bookkeeping():
    """The fold statement the GPU tests compare with, on a hand-made case: env 0 falls, env 1 times out,
    env 2 is reset with an empty running row (not an episode), env 3 runs on."""
    run = np.zeros((13, 4))
    run[:, 0] = np.arange(1, 14)
    run[:, 1] = 2 * np.arange(1, 14)
    run[:, 3] = 5.0
    done = np.ones((13, 4))
    done[12] = (20.0, 20.0, 0.0, 0.0)
    counts = np.zeros((4, 4), np.int64)
    r, d, c = MR.fold(run, done, counts, 0, reset=[1, 1, 1, 0], time_out=[0, 1, 0, 0])
    assert c.tolist() == [[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert d[:12, 0].tolist() == (1 + np.arange(1, 13)).tolist() and d[12, 0] == 20.0   # max(20, 13)
    assert d[12, 1] == 26.0 and d[:, 2].tolist() == [1.0] * 12 + [0.0]
    assert not r[:, :3].any() and (r[:, 3] == 5.0).all() and (d[:12, 3] == 1.0).all()
    r2, d2, c2 = MR.fold(run, done, counts, 1, mask=[0, 1, 0, 1])
    assert (r2[:, 0] == run[:, 0]).all() and not r2[:, 1].any() and not r2[:, 3].any()
    assert np.array_equal(d2, done) and not c2.any()
    r3, _, _ = MR.fold(run, done, counts, 1)
    assert not r3.any()


# ---------------------------------------------------------------- wrong samples
# (name, the text replaced, its replacement, rows that must fail)
WRONG = [
    ("contact_ge", "if (fz[f] > HG_METRICS_CONTACT_Z) {", "if (fz[f] >= HG_METRICS_CONTACT_Z) {", ["force_5_and_next"]),
    ("clamp_on_the_sum", "work += p > 0.0 ? p : 0.0;", "work += p;", ["mixed_power"]),
    ("quat_not_normalised", "const double qn = 1.0 / sqrt(", "const double qn = 1.0 + 0.0 * sqrt(", ["quat_unnormalised"]),
    ("rotate_forward", "out[0] = v[0] * s - w2 * cx + d * x;", "out[0] = v[0] * s + w2 * cx + d * x;",
     ["walking", "pitched_yawed"]),
    ("float_accumulation", "const double p = tau[j] * qd[j];", "const double p = (float)(tau[j] * qd[j]);", ["walking"]),
    ("limit_of_joint_0", "(double)torque_limit[j];", "(double)torque_limit[0];", ["torque_at_limit"]),
]


@pytest.fixture(scope="module")
def wrong(tmp_path_factory, host):
    out = tmp_path_factory.mktemp("metrics_wrong")
    text = open(HEADER).read()
    jobs = []
    for name, old, new, _ in WRONG:
        assert text.count(old) == 1, f"{name}: the replaced text matches {text.count(old)} times"
        src = os.path.join(str(out), f"hg_metrics_sample_{name}.h")
        with open(src, "w") as f:
            f.write(text.replace(old, new))
        jobs.append((name, src))
    with ThreadPoolExecutor(3) as ex:
        libs = list(ex.map(lambda j: _compile(out, j[0], j[1]), jobs))
    return {name: L for (name, _), L in zip(jobs, libs)}


@pytest.mark.parametrize("name", [w[0] for w in WRONG])
def test_wrong_sample_fails_the_table(wrong, name):
    """The table sees a one-line mistake: the named rows leave the bound."""
    expect = next(w[3] for w in WRONG if w[0] == name)
    n = len(MC.ROWS)
    st = MC.stack(range(n))
    zero, zc = np.zeros((13, n)), np.zeros((4, n), np.int64)
    ref, _ = MR.sample(st, MC.TORQUE_LIMIT, MC.DT, zero, zc)
    r, _, _ = host_sample(wrong[name], st, zero, zc)
    bad = [MC.NAMES[e] for e in range(n) if MR.max_deviation(r[:, e], ref[:, e]) > 1.0]
    print(f"{name}: fails {bad}")
    assert set(expect) <= set(bad), f"{name}: passes {sorted(set(expect) - set(bad))}"


# ---------------------------------------------------------------- config and ABI
def test_switch_is_off_by_default_and_reaches_hg_cfg():
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    assert cfg.metrics.gait is False
    _, js = N.load_model()
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.gait_metrics == 0
    cfg.metrics.gait = True
    hc, _ = build_hg_cfg(cfg, 16, cfg.sim.dt, 5, js)
    assert hc.gait_metrics == 1
    # the switch fills the padding in front of critic_height_points: no other field moved
    F = N.HgCfg
    assert F.gait_metrics.offset == F.critic_height_scale.offset + 4 == F.critic_height_points.offset - 4
    assert N.METRICS_NAMES == MR.NAMES and N.METRICS_COUNT_NAMES == MR.COUNT_NAMES
    import humanoid.scripts.sim2sim as S2S
    assert S2S.make_cfg("urdf", 4, duration=1.0).metrics.gait is False


def test_header_declares_the_entry_points_and_ids(tmp_path):
    from humanoid import _native as N
    src = open(os.path.join(REPO, "include", "hgsim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("hg_metrics_sample", "hg_metrics_fold", "hg_metrics_clear"):
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", code, flags=re.M), name
        assert name in N.EXPORTS
    for name in MR.NAMES:                      # the header documents every slot
        assert re.search(r"slot\s+%d\s+%s\b" % (MR.NAMES.index(name), name), src), name
    ids = ["METRICS_RUN", "METRICS_DONE", "METRICS_COUNT"]
    assert [N.T[k] - N.T[ids[0]] for k in ids] == [0, 1, 2]
    c = tmp_path / "ids.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hgsim.h"\nint main(){printf("%d %d %d %d %zu %zu",'
                 'HG_T_METRICS_RUN,HG_T_METRICS_DONE,HG_T_METRICS_COUNT,HG_T_COUNT,offsetof(hg_cfg,gait_metrics),'
                 'sizeof(hg_cfg));}')
    exe = tmp_path / "ids"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [N.T[k] for k in ids] + [len(N.TENSOR_IDS), N.HgCfg.gait_metrics.offset, ctypes.sizeof(N.HgCfg)]


def test_library_refuses_and_sizes_without_a_gpu():
    """No GPU needed: a NULL sim is refused with a reason before any launch; the arena grows by the
    three buffers only when the switch is on."""
    from humanoid import _native as N
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    L = N.load_library()
    assert L.hg_metrics_sample(None, None) == 1 and b"hg_metrics_sample: sim is NULL" in L.hg_last_error(None)
    assert L.hg_metrics_fold(None, 0, None, None) == 1 and b"hg_metrics_fold" in L.hg_last_error(None)
    assert L.hg_metrics_clear(None, None) == 1 and b"hg_metrics_clear" in L.hg_last_error(None)
    c = N.HgCfg()
    c.num_envs, c.frame_stack, c.c_frame_stack = 65, 15, 3
    base = L.hg_arena_bytes(ctypes.byref(c))
    c.gait_metrics = 1
    grown = L.hg_arena_bytes(ctypes.byref(c))
    assert grown - base == 2 * 13 * 128 * 8 + 4 * 128 * 4       # np = 128: two f64 [13, np], one i32 [4, np]


# ---------------------------------------------------------------- gait_report's arithmetic
def test_gait_report_on_hand_made_accumulators():
    from humanoid.envs.custom.humanoid_env import gait_report_arrays, gait_report_row
    s = MR.NAMES.index
    done = np.zeros((13, 3))
    counts = np.zeros((4, 3), np.int64)
    # env 0: 2 episodes, 100 steps, 4 m; env 1: 1 episode, 50 steps, 1 m; env 2: nothing completed
    done[s("steps")] = (100, 50, 0)
    done[s("err_vx2")] = (4.0, 2.0, 0)
    done[s("err_vy2")] = (1.0, 0.5, 0)
    done[s("err_wz2")] = (9.0, 4.5, 0)
    done[s("distance")] = (4.0, 1.0, 0)
    done[s("work_pos")] = (800.0, 300.0, 0)
    done[s("torque2")] = (30.0, 15.0, 0)
    done[s("tilt2")] = (1.0, 0.5, 0)
    done[s("slip")] = (0.2, 0.3, 0)
    done[s("action_rate2")] = (25.0, 12.5, 0)
    done[s("double_support")] = (20, 10, 0)
    done[s("flight")] = (5, 10, 0)
    done[s("peak_torque")] = (0.8, 1.25, 0)
    counts[:, 0] = (2, 1, 1, 0)
    counts[:, 1] = (1, 1, 0, 3)
    counts[:, 2] = (0, 0, 0, 4)
    mass, g, dt = np.array([50.0, 60.0, 70.0]), 9.81, 0.01
    r = gait_report_row(done, counts, mass, g, dt)
    assert (r["episodes"], r["falls"], r["time_outs"], r["skipped"], r["steps"]) == (3, 2, 1, 7, 150)
    assert r["fall_rate"] == 2 / 3
    assert r["rms_err_vx"] == np.sqrt(6.0 / 150) and r["rms_err_vy"] == np.sqrt(1.5 / 150)
    assert r["rms_err_wz"] == np.sqrt(13.5 / 150)
    assert r["distance_per_episode"] == 5.0 / 3
    assert r["cost_of_transport"] == 1100.0 / (50.0 * g * 4.0 + 60.0 * g * 1.0 + 70.0 * g * 0.0)
    assert r["slip_per_metre"] == 0.5 / 5.0
    assert r["tilt_rms"] == np.sqrt(1.5 / 150)
    assert r["double_support_fraction"] == 30 / 150 and r["flight_fraction"] == 15 / 150
    assert r["peak_torque_ratio"] == 1.25
    assert r["mean_torque2"] == 45.0 / (150 * dt) and r["action_rate_rms"] == np.sqrt(37.5 / 150)
    # per terrain type: envs 0 and 2 are type 4, env 1 type 1
    by = gait_report_arrays(done, counts, mass, g, dt, terrain_types=[4, 1, 4])
    assert by["overall"] == r and sorted(by["terrain_types"]) == [1, 4]
    assert by["terrain_types"][1]["episodes"] == 1 and by["terrain_types"][1]["fall_rate"] == 1.0
    assert by["terrain_types"][1]["cost_of_transport"] == 300.0 / (60.0 * g * 1.0)
    assert by["terrain_types"][4]["episodes"] == 2 and by["terrain_types"][4]["skipped"] == 4
    assert by["terrain_types"][4]["rms_err_vx"] == np.sqrt(4.0 / 100)


def test_gait_report_with_no_episode_gives_none():
    from humanoid.envs.custom.humanoid_env import gait_report_arrays
    counts = np.zeros((4, 5), np.int64)
    counts[3] = 2
    r = gait_report_arrays(np.zeros((13, 5)), counts, np.full(5, 50.0), 9.81, 0.01)
    assert r["episodes"] == 0 and r["falls"] == 0 and r["skipped"] == 10 and r["steps"] == 0
    for k in ("fall_rate", "rms_err_vx", "rms_err_vy", "rms_err_wz", "distance_per_episode", "cost_of_transport",
              "slip_per_metre", "tilt_rms", "double_support_fraction", "flight_fraction", "peak_torque_ratio",
              "mean_torque2", "action_rate_rms"):
        assert r[k] is None, k
    # episodes that went nowhere: distance-based figures are None, the others are numbers
    done = np.zeros((13, 5))
    done[0] = 10
    counts[0] = 1
    counts[2] = 1
    r = gait_report_arrays(done, counts, np.full(5, 50.0), 9.81, 0.01)
    assert r["cost_of_transport"] is None and r["slip_per_metre"] is None
    assert r["fall_rate"] == 0.0 and r["rms_err_vx"] == 0.0 and r["distance_per_episode"] == 0.0


def test_evaluate_formats_a_report_and_builds_its_cfg():
    """scripts/evaluate.py without a GPU: the table has a row per figure, a column per terrain type
    (one column when there is a single type), '-' for None; the cfg turns the metrics on and a fixed
    command turns resampling and the heading command off."""
    from humanoid.envs.custom.humanoid_env import gait_report_arrays
    from humanoid.scripts import evaluate as EV
    done = np.zeros((13, 4))
    done[0] = (10, 20, 0, 30)
    done[4] = (1.0, 2.0, 0, 0.5)
    done[5] = (400.0, 900.0, 0, 100.0)
    counts = np.zeros((4, 4), np.int64)
    counts[0] = (1, 2, 0, 1)
    counts[1] = (1, 0, 0, 1)
    counts[2] = (0, 2, 0, 0)
    rep = gait_report_arrays(done, counts, np.full(4, 50.0), 9.81, 0.01, terrain_types=[0, 0, 3, 3])
    text = EV.format_report(rep)
    lines = text.splitlines()
    assert lines[0].split() == ["overall", "type", "0", "type", "3"]
    row = {ln.split()[0]: ln.split()[1:] for ln in lines[1:]}
    assert set(row) == set(rep["overall"]) and row["episodes"] == ["4", "3", "1"]
    assert row["fall_rate"] == ["0.5000", "0.3333", "1.0000"]
    one = gait_report_arrays(np.zeros((13, 2)), np.zeros((4, 2), np.int64), np.full(2, 50.0), 9.81, 0.01, terrain_types=[0, 0])
    lines = EV.format_report(one).splitlines()
    assert lines[0].split() == ["overall"] and all(ln.split()[1] in ("-", "0") for ln in lines[1:])
    cfg = EV.make_cfg(16, 5.0, command=(0.4, 0.0, 0.1), terrain="plane", seed=7)
    assert cfg.metrics.gait is True and cfg.env.num_envs == 16 and cfg.seed == 7
    assert cfg.commands.heading_command is False and cfg.commands.resampling_time > 5.0 + cfg.env.episode_length_s
    free = EV.make_cfg(16, 5.0)
    from humanoid.envs import XBotLCfg
    assert free.commands.resampling_time == XBotLCfg().commands.resampling_time and free.metrics.gait is True
    with pytest.raises(ValueError):
        EV.make_cfg(16, 5.0, command=(0.4, 0.0))


def test_a_single_terrain_type_is_the_overall_row_exactly():
    """The same envs give the same figures to the last bit, whole array or a type's selection (the
    sums run over C-contiguous copies: numpy's order follows the memory layout)."""
    from humanoid.envs.custom.humanoid_env import gait_report_arrays
    rs = np.random.RandomState(8)
    for n in (3, 8, 65, 200):
        packed = rs.uniform(0.0, 7.0, (19, n))         # rows of a wider array, as the env's packed copy
        packed[0] = rs.randint(1, 90, n)
        counts = rs.randint(1, 4, (4, n))
        rep = gait_report_arrays(packed[:13], counts, rs.uniform(40, 60, n), 9.81, 0.01, terrain_types=np.zeros(n, np.int64))
        assert rep["terrain_types"][0] == rep["overall"], n
