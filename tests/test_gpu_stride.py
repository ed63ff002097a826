"""Stride statistics on the GPU: k_stride_sample / k_stride_fold (run by hg_metrics_sample /
hg_metrics_fold / hg_metrics_clear when hg_cfg.gait_metrics has bit 1) against the float64 reference of
tests/stride_ref.py on the planted sequences of tests/stride_cases.py, on an env's own generated
heightfield and on a driven env; where env.step() and reset_idx put the calls; a captured graph; that
the switch off leaves nothing behind; the runner's, evaluate's and play's figures.

Bounds as in tests/test_stride_cases.py: counts and every state slot exactly, the float sums relative
1e-12 with absolute 1e-15 (metrics_ref.RTOL / ATOL), at most 100 accumulated steps.  Env counts 1, 3
and 65 (np = 128: the second wave is partly filled).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import metrics_ref as MR
import stride_cases as SC
import stride_ref as SR
from test_gpu_parity import _make_env, _need_gpu

pytestmark = pytest.mark.gpu

f32 = np.float32
BUFFERS = (("STRIDE_RUN", 2 * SR.NS), ("STRIDE_DONE", 2 * SR.NS), ("STRIDE_STATE", 2 * SR.NST))
PAD = 1234.5625                      # planted into the padding columns: they must keep it


def _g(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _lib():
    from humanoid import _native as N
    return N, N.lib()


def _stream(env):
    return ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)


def _plant(env, state):
    for k in SR.STATE_KEYS:
        getattr(env, k).copy_(torch.from_numpy(np.ascontiguousarray(state[k])).to(env.device))


def _read(env):
    torch.cuda.synchronize()
    return {k: getattr(env, k).detach().cpu().numpy().copy() for k in SR.STATE_KEYS}


def _acc(env):
    return _g(env.stride_state), _g(env.stride_running), _g(env.stride_completed)


def _whole(env, tid, rows):
    """The whole [rows, np] buffer behind a stride view as a device tensor, padding columns included."""
    N, L = _lib()
    d = N.HgDesc()
    N.check(L.hg_tensor(env.sim, N.T[tid], ctypes.byref(d)), env.sim)
    np_ = int(d.strides[0])
    return env._arena_base.view(torch.float64).as_strided([rows, np_], [np_, 1], d.offset_bytes // 8)


def _stride_env(n, **over):
    env = _make_env(n, metrics__gait=True, metrics__strides=True, **over)
    assert tuple(env._hgcfg.feet_body) == SC.FEET and int(env._hgcfg.gait_metrics) == 3
    assert float(env._hgcfg.sim_dt) * int(env._hgcfg.decimation) == SC.DT
    env.clear_gait_metrics()
    return env


def _compare(label, got, want, worst):
    """got / want: (state, run, done)."""
    assert all(np.isfinite(a).all() for a in got), label
    try:
        worst[0] = max(worst[0], SR.compare(got[0], got[1], want[0], want[1]))
        worst[0] = max(worst[0], SR.compare(got[0], got[2], want[0], want[2]))
    except AssertionError as err:
        raise AssertionError(f"{label}: {err}") from None
    assert worst[0] <= 1.0, f"{label}: sums deviate {worst[0]:.3e} x the bound"


def _drive_planted(env, seq, terrain, resets, worst, label, check_every=8):
    """Plant each sample, hg_metrics_sample + hg_metrics_fold(0) with planted reset flags, the
    reference alongside; compared every few samples and at the end.  Returns the reference triple."""
    N, L = _lib()
    T, n = seq["root_states"].shape[:2]
    ref = [np.zeros((2 * SR.NST, n)), np.zeros((2 * SR.NS, n)), _g(env.stride_completed)]
    s = _stream(env)
    for t in range(T):
        state = {k: seq[k][t] for k in SR.STATE_KEYS}
        _plant(env, state)
        env._reset_u8.copy_(torch.from_numpy(resets[t].astype(np.uint8)).to(env.device))
        assert L.hg_metrics_sample(env.sim, s) == 0
        assert L.hg_metrics_fold(env.sim, 0, None, s) == 0
        ref[0], ref[1], _ = SR.sample(state, terrain, SC.DT, ref[0], ref[1])
        ref[:] = SR.fold(ref[0], ref[1], ref[2], 0, reset=resets[t])
        if t % check_every == check_every - 1 or t == T - 1:
            _compare(f"{label} sample {t}", _acc(env), ref, worst)
    return ref


def _resets(T, n):
    """Env e is reset at sample 13 + (e % 9) * 3 (mid-swing for some sequences, in stance for others)
    and every env at the last sample, so every running sum ends in the completed rows."""
    r = np.zeros((T, n), bool)
    for e in range(n):
        if e % 2 == 1:
            r[13 + (e % 9) * 3, e] = True
    r[T - 1] = True
    return r


# ---------------------------------------------------------------- planted sequences
@pytest.mark.parametrize("n", [1, 3, 65])
def test_planted_sequences(n):
    """Every planted sequence through the kernels: n = 65 runs them all at once (env e sees sequence
    e mod the count), n = 3 in rounds of three, n = 1 the walk, the chatter and a non-finite gap one
    after the other.  RUN, DONE and STATE against the reference; the padding columns keep their bits."""
    _need_gpu()
    N, L = _lib()
    env = _stride_env(n)
    for tid, rows in BUFFERS:
        _whole(env, tid, rows)[:, n:] = PAD
    names, seq = SC.group("plane")
    C = len(names)
    if n == 1:
        rounds = [[names.index(k)] for k in ("clean_walk", "swing_1_2_3", "nan_rigid_pos")]
    elif n == 3:
        rounds = [[(3 * r + e) % C for e in range(3)] for r in range(-(-C // 3))]
    else:
        rounds = [[e % C for e in range(n)]]
    worst = [0.0]
    total = np.zeros(2 * SR.NS)
    for r, idx in enumerate(rounds):
        sub = {k: seq[k][:, idx] for k in SR.STATE_KEYS}
        ref = _drive_planted(env, sub, None, _resets(SC.T, n), worst, f"n={n} round {r}")
        assert not ref[0].any() and not ref[1].any()          # the last sample's reset folded everything
        total = ref[2].sum(axis=1)
    print(f"planted sequences, n = {n}: {len(rounds)} rounds, largest deviation {worst[0]:.3e} x the bound (rtol {MR.RTOL}, "
          f"atol {MR.ATOL}); completed strides {total[0]:.0f} + {total[SR.NS]:.0f}, short swings "
          f"{total[SR.NS - 1]:.0f} + {total[2 * SR.NS - 1]:.0f}")
    assert total[0] + total[SR.NS] > 0
    for tid, rows in BUFFERS:
        full = _g(_whole(env, tid, rows))
        assert full.shape[1] == (n + 63) // 64 * 64 and (full[:, n:] == PAD).all(), tid
    # the discard: a mask, then NULL; nothing is added to the completed rows
    sub = {k: seq[k][:, [e % C for e in range(n)]] for k in SR.STATE_KEYS}
    none = np.zeros((SC.T, n), bool)
    ref = _drive_planted(env, {k: v[:20] for k, v in sub.items()}, None, none[:20], worst, f"n={n} before the discard")
    assert ref[0].any()
    mask = np.arange(n) % 2 == 0
    m = torch.from_numpy(mask.astype(np.uint8)).to(env.device)
    assert L.hg_metrics_fold(env.sim, 1, ctypes.c_void_p(m.data_ptr()), _stream(env)) == 0
    ref[:] = SR.fold(ref[0], ref[1], ref[2], 1, mask=mask)
    _compare(f"n={n} discard masked", _acc(env), ref, worst)
    assert L.hg_metrics_fold(env.sim, 1, None, _stream(env)) == 0
    ref[:] = SR.fold(ref[0], ref[1], ref[2], 1)
    _compare(f"n={n} discard all", _acc(env), ref, worst)
    assert not ref[0].any() and not ref[1].any() and ref[2].any()
    for tid, rows in BUFFERS:
        assert (_g(_whole(env, tid, rows))[:, n:] == PAD).all(), tid
    env.clear_gait_metrics()
    assert not any(a.any() for a in _acc(env))


# ---------------------------------------------------------------- the env's own heightfield
def test_planted_feet_on_the_generated_heightfield():
    """Feet planted on an env's generated terrain: the kernel reads hg_cfg's heightfield, the
    reference the env's own height_samples array.  The walks start where the field is steepest, far
    outside it (clamped) and in its middle."""
    _need_gpu()
    n = 3
    env = _stride_env(n, terrain__mesh_type="heightfield")
    c = env._hgcfg
    hf = _g(env.height_samples)
    assert c.terrain_type == 1 and hf.shape == (c.hf_rows, c.hf_cols) and c.heightfield == env.height_samples.data_ptr()
    terrain = dict(hf=hf, hs=f32(c.hf_horizontal_scale), vs=f32(c.hf_vertical_scale), border=f32(c.hf_border))
    hs, border = float(c.hf_horizontal_scale), float(c.hf_border)
    jump = np.abs(np.diff(hf.astype(np.int64), axis=0))
    i, j = np.unravel_index(np.argmax(jump), jump.shape)
    assert jump[i, j] > 0
    # the first walk's left foot (origin y + HALF_WIDTH) walks along column j towards the jump between rows i and i + 1
    starts = [((i - 1) * hs - border, j * hs - border + 0.02 - SC.HALF_WIDTH), (-1e4, 3e4),
              ((hf.shape[0] // 2) * hs - border, (hf.shape[1] // 2) * hs - border)]
    pat = SC._pat("S3 W8 S9 W8 S12", "S12 W8 S9 W8 S3")
    gz = lambda x, y: float(SR.ground(f32(x), f32(y), terrain))  # noqa: E731
    seqs = [SC.gait(pat, origin=o, speed=1.5, ground_z=gz, seed=40 + k) for k, o in enumerate(starts)]
    seq = {k: np.stack([s[k] for s in seqs], axis=1) for k in SR.STATE_KEYS}
    heights = {float(SR.ground(seq["rigid_state"][t, 0, SC.FEET[0], 0], seq["rigid_state"][t, 0, SC.FEET[0], 1], terrain))
               for t in range(SC.T)}
    assert len(heights) > 1, "the first walk stays on one height"
    worst = [0.0]
    ref = _drive_planted(env, seq, terrain, _resets(SC.T, n), worst, "heightfield", check_every=4)
    on_plane = SR.replay(seq, None, SC.DT)[1]
    i_c = SR.NAMES.index("clearance")
    print(f"heightfield: largest deviation {worst[0]:.3e} x the bound; heights under foot 0 of env 0: {sorted(heights)}; "
          f"clearance sums {ref[2][i_c]} (on a plane {on_plane[i_c]})")
    assert ref[2][0].sum() >= 4
    assert abs(ref[2][i_c, 0] - on_plane[i_c, 0]) > 1e-3       # the terrain rule matters for the walk across the jump


# ---------------------------------------------------------------- wiring
STEPS, TIMEOUT_AT, TIP_AT, RESET_AT, LATE_TIMEOUT_AT = 60, 6, 3, 31, 45
RESET_IDS = [0, 7, 40]


def _actions(k, n, device):
    g = torch.Generator().manual_seed(2000 + k)
    return (0.6 * torch.randn(n, 12, generator=g)).to(device)


def _intervene(env, k):
    """Before step k: env 1 is put one step from its time-out, env 2 is tipped onto its side just
    above the ground (a fall within a few steps); late in the run every fourth env times out, so
    that running sums of walking envs are folded into the completed rows."""
    if k == TIMEOUT_AT:
        env.episode_length_buf[1] = int(env.max_episode_length)
    if k == LATE_TIMEOUT_AT:
        env.episode_length_buf[3::4] = int(env.max_episode_length)
    if k == TIP_AT:
        root = env.root_states[2].clone()
        root[2] = env.env_origins[2, 2] + 0.24
        root[3:7] = torch.tensor([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)], dtype=torch.float32)
        root[7:13] = 0.0
        env.root_states[2] = root


def test_wiring_manual_sequence_twin_step_and_graph():
    """65 envs driven through the ABI for 60 steps of random actions (hg_step, read the views,
    hg_metrics_sample, hg_post, hg_metrics_fold) with a forced time-out, a forced fall and a reset_idx
    in the middle: the reference replayed from what was read gives the device's stride buffers; a twin
    env driven through env.step() / env.reset_idx() alone ends with the same bits; a captured
    sample + fold pair replays to what the direct calls give."""
    _need_gpu()
    N, L = _lib()
    n = 65
    env, twin = _stride_env(n), _stride_env(n)
    dt = float(env._hgcfg.sim_dt) * int(env._hgcfg.decimation)
    feet = tuple(env._hgcfg.feet_body)
    ref = [np.zeros((2 * SR.NST, n)), np.zeros((2 * SR.NS, n)), np.zeros((2 * SR.NS, n))]
    for a in _acc(env) + _acc(twin):      # creation's reset discarded, nothing counted
        assert not a.any()
    s = _stream(env)
    mask_np = np.zeros(n, bool)
    mask_np[RESET_IDS] = True
    mask = torch.from_numpy(mask_np.astype(np.uint8)).to(env.device)
    discarded = None
    for k in range(STEPS):
        act = _actions(k, n, env.device)
        for e_ in (env, twin):
            _intervene(e_, k)
        if k == RESET_AT:
            discarded = ref[0][:, RESET_IDS].copy()
            N.check(L.hg_reset_masked(env.sim, ctypes.c_void_p(mask.data_ptr()), ctypes.c_uint64(env.common_step_counter), s), env.sim)
            N.check(L.hg_metrics_fold(env.sim, 1, ctypes.c_void_p(mask.data_ptr()), s), env.sim)
            ref[:] = SR.fold(ref[0], ref[1], ref[2], 1, mask=mask_np)
            twin.reset_idx(RESET_IDS)
            st_now = _g(twin.stride_state)
            assert not st_now[:, RESET_IDS].any() and st_now.any()         # reset_idx discards the running stride
        N.check(L.hg_step(env.sim, ctypes.c_void_p(act.data_ptr()), ctypes.c_uint64(env.common_step_counter), s), env.sim)
        env.common_step_counter += 1
        st = _read(env)
        N.check(L.hg_metrics_sample(env.sim, s), env.sim)
        N.check(L.hg_post(env.sim, ctypes.c_uint64(env.common_step_counter), s), env.sim)
        N.check(L.hg_metrics_fold(env.sim, 0, None, s), env.sim)
        reset = _g(env._reset_u8)
        ref[0], ref[1], _ = SR.sample(st, None, dt, ref[0], ref[1], feet)
        ref[:] = SR.fold(ref[0], ref[1], ref[2], 0, reset=reset)
        twin.step(act)
    got = _acc(env)
    worst = [0.0]
    _compare("wiring", got, ref, worst)
    tot = (got[1] + got[2]).sum(axis=1)
    print(f"wiring: {STEPS} steps x {n} envs, largest deviation {worst[0]:.3e} x the bound; strides {tot[0]:.0f} + "
          f"{tot[SR.NS]:.0f}, pairs {tot[6]:.0f} + {tot[SR.NS + 6]:.0f}, short swings {tot[9]:.0f} + {tot[SR.NS + 9]:.0f}; "
          f"completed rows of {int((got[2].any(axis=0)).sum())} envs hold sums")
    assert discarded is not None and discarded.any(), "the reset envs had no detector state to discard"
    assert tot[0] + tot[SR.NS] + tot[9] + tot[SR.NS + 9] > 0, "no foot ever left the ground and came back"
    assert got[0].any() and got[2].any(), "no running sum was ever folded into the completed rows"
    for name, a, b in zip(("state", "running", "completed"), got, _acc(twin)):
        assert a.tobytes() == b.tobytes(), f"env.step() and the manual sequence differ in the stride {name} rows"
    rep = twin.stride_report(by_terrain_type=True)
    assert sorted(rep["terrain_types"]) == [0] and rep["terrain_types"][0] == rep["overall"]
    assert rep["overall"]["both"]["strides"] == int(got[2][0].sum() + got[2][SR.NS].sum())
    assert all(v is None or np.isfinite(v) for row in rep["overall"].values() for v in row.values())
    # a captured sample + fold pair: `twin` replays a graph where `env` makes the direct calls; both
    # hold the same state, so the same bits come out
    for k_ in SR.STATE_KEYS:
        assert torch.equal(getattr(env, k_), getattr(twin, k_)), k_
    views = lambda e_: (e_.stride_state, e_.stride_running, e_.stride_completed)  # noqa: E731
    before = [a.clone() for a in views(twin)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cs = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            N.check(L.hg_metrics_sample(twin.sim, cs), twin.sim)
            N.check(L.hg_metrics_fold(twin.sim, 0, None, cs), twin.sim)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(views(twin), before))       # captured, not run
    N.check(L.hg_metrics_sample(env.sim, s), env.sim)
    N.check(L.hg_metrics_fold(env.sim, 0, None, s), env.sim)
    graph.replay()
    torch.cuda.synchronize()
    for name, a, b in zip(("state", "running", "completed"), _acc(env), _acc(twin)):
        assert a.tobytes() == b.tobytes(), f"graph replay and direct calls differ in the stride {name} rows"
    assert not torch.equal(twin.stride_state, before[0])                       # the pair did advance the detector
    assert _g(twin.metrics_running).tobytes() == _g(env.metrics_running).tobytes()


# ---------------------------------------------------------------- off means off
def test_off_means_off():
    """metrics.gait on, metrics.strides off: the new views do not exist, hg_tensor refuses the ids, the
    arena is the size it always was, and over 16 steps the env's outputs and the three metrics buffers
    are bitwise those of an env with the strides on (the stride kernels only read what the parent's
    kernels wrote, and write their own buffers) and of a default env."""
    _need_gpu()
    N, L = _lib()
    n = 65
    plain = _make_env(n)
    off = _make_env(n, metrics__gait=True)
    on = _stride_env(n)
    for name in ("stride_running", "stride_completed", "stride_state", "stride_names", "stride_report"):
        assert not hasattr(off, name) and not hasattr(plain, name) and hasattr(on, name), name
    assert on.stride_names == SR.NAMES and int(off._hgcfg.gait_metrics) == 1
    assert tuple(on.stride_running.shape) == tuple(on.stride_completed.shape) == (2 * SR.NS, n)
    assert tuple(on.stride_state.shape) == (2 * SR.NST, n) and on.stride_state.dtype == torch.float64
    assert on.stride_running.stride() == (128, 1)                       # zero-copy views of the SoA arena
    d = N.HgDesc()
    for tid, _ in BUFFERS:
        for e_ in (off, plain):
            assert L.hg_tensor(e_.sim, N.T[tid], ctypes.byref(d)) == 1
            assert b"stride statistics are off" in L.hg_last_error(e_.sim)
        assert L.hg_tensor(on.sim, N.T[tid], ctypes.byref(d)) == 0 and d.dtype == 4
    assert on._arena_base.numel() - off._arena_base.numel() == 2 * 20 * 128 * 8 + 16 * 128 * 8
    assert off._arena_base.numel() - plain._arena_base.numel() == 2 * 13 * 128 * 8 + 4 * 128 * 4
    # hg_update_cfg compares the whole value: 1 -> 3 would change the layout
    c = type(off._hgcfg).from_buffer_copy(off._hgcfg)
    c.gait_metrics = 3
    assert L.hg_update_cfg(off.sim, ctypes.byref(c), _stream(off)) == 1 and b"layout" in L.hg_last_error(off.sim)
    for k in range(16):
        act = _actions(k, n, off.device)
        outs = [e_.step(act) for e_ in (plain, off, on)]
        for x, y, z in zip(*[o[:4] for o in outs]):
            assert torch.equal(x, y) and torch.equal(y, z), f"step {k}"
    for attr in ("root_states", "dof_pos", "dof_vel", "torques", "commands", "contact_forces", "rigid_state"):
        assert torch.equal(getattr(off, attr), getattr(on, attr)) and torch.equal(getattr(off, attr), getattr(plain, attr)), attr
    for attr in ("metrics_running", "metrics_completed", "metrics_counts"):
        assert _g(getattr(off, attr)).tobytes() == _g(getattr(on, attr)).tobytes(), attr
    assert int(_g(off.metrics_running)[0].sum() + _g(off.metrics_completed)[0].sum()) == 16 * n
    assert _g(on.stride_state).any()
    with pytest.raises(ValueError, match="metrics.strides needs metrics.gait"):
        _make_env(2, metrics__strides=True)


# ---------------------------------------------------------------- runner, evaluate, play
def _runner(env, log_dir, steps=16):
    from humanoid.algo.ppo import OnPolicyRunner
    from humanoid.envs import XBotLCfgPPO
    from humanoid.utils.helpers import class_to_dict
    tcfg = XBotLCfgPPO()
    tcfg.runner.num_steps_per_env = steps
    return OnPolicyRunner(env, class_to_dict(tcfg), log_dir=log_dir, device="cuda:0")


def test_runner_reports_stride_stats(tmp_path):
    """One learn iteration with the switch on (0.1 s episodes, so the rollout completes episodes) puts
    stride_* entries into last_iteration_stats and Gait/stride_* scalars into the log, next to the
    gait_* ones; the lazy path without a log writer delivers them too; with the switch off (gait on)
    no stride key appears."""
    _need_gpu()
    from humanoid.algo.ppo.on_policy_runner import _JsonlWriter
    over = dict(metrics__gait=True, env__episode_length_s=0.1)
    env = _make_env(64, metrics__strides=True, **over)
    log_dir = str(tmp_path / "run")
    runner = _runner(env, log_dir)
    runner.writer = _JsonlWriter(log_dir)
    runner.learn(1, init_at_random_ep_len=True)
    stats = runner.last_iteration_stats
    strides = {k: v for k, v in stats.items() if k.startswith("stride_")}
    print("runner stride stats:", strides)
    assert "stride_strides" in strides and "stride_strides_per_episode" in strides and "gait_episodes" in stats
    assert all(np.isfinite(v) for v in strides.values()) and not any(k.startswith("gait_stride") for k in stats)
    tags = {json.loads(ln)["tag"] for ln in open(os.path.join(log_dir, "scalars.jsonl"))}
    assert {"Gait/stride_strides", "Gait/stride_strides_per_episode", "Gait/episodes"} <= tags
    assert not _g(env.stride_completed).any()                                # a fresh interval
    lazy = _runner(_make_env(64, metrics__strides=True, **over), None)
    lazy.learn(2, init_at_random_ep_len=True)
    assert "stride_strides" in lazy.last_iteration_stats and "gait_episodes" in lazy.last_iteration_stats
    off = _runner(_make_env(64, **over), str(tmp_path / "off"))
    off.writer = _JsonlWriter(str(tmp_path / "off"))
    off.learn(1, init_at_random_ep_len=True)
    assert "gait_episodes" in off.last_iteration_stats
    assert not any(k.startswith("stride_") for k in off.last_iteration_stats)
    tags = {json.loads(ln)["tag"] for ln in open(os.path.join(str(tmp_path / "off"), "scalars.jsonl"))}
    assert "Gait/episodes" in tags and not any("stride" in t for t in tags)


def test_evaluate_reports_strides(tmp_path, capsys):
    """scripts/evaluate.py --strides adds a "strides" section (overall and per terrain type) to the
    report and the JSON; without the flag the report and the printed table are what they were."""
    _need_gpu()
    from humanoid.scripts import evaluate as EV
    actor = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hg_trained_actor.npz")
    args = ["--load_model", actor, "--envs", "8", "--duration", "0.3", "--command", "0.4", "0", "0"]
    plain = EV.main(args + ["--out", str(tmp_path / "plain")])
    out_plain = capsys.readouterr().out
    rep = EV.main(args + ["--out", str(tmp_path / "strides"), "--strides"])
    out_strides = capsys.readouterr().out
    assert sorted(plain) == ["overall", "settings", "terrain_types"] and "mean_clearance" not in out_plain
    assert sorted(rep) == ["overall", "settings", "strides", "terrain_types"] and "mean_clearance" in out_strides
    assert rep["overall"] == plain["overall"] and rep["settings"] == plain["settings"]      # the same run otherwise
    assert out_strides.startswith(out_plain.rsplit("\n", 2)[0])
    js = json.load(open(tmp_path / "strides" / "gait_report.json"))
    assert js["strides"]["overall"] == rep["strides"]["overall"] and list(js["strides"]["terrain_types"]) == ["0"]
    assert "strides" not in json.load(open(tmp_path / "plain" / "gait_report.json"))
    assert sorted(rep["strides"]["overall"]) == ["both", "left", "right"]
    with pytest.raises(ValueError):
        EV.evaluate(lambda o: o[:, :12], duration=0.1, env=_make_env(2, metrics__gait=True), strides=True)
    env = _make_env(8, metrics__gait=True, metrics__strides=True, env__episode_length_s=0.2)
    rep2, env = EV.evaluate(lambda o: torch.zeros(o.shape[0], 12, device=o.device), duration=0.5, env=env, strides=True)
    text = EV.format_stride_report(rep2["strides"])
    print(text)
    assert text.splitlines()[0].split() == ["overall", "left", "right", "both"]
    assert rep2["overall"]["episodes"] >= 8 and rep2["strides"]["overall"]["both"]["strides"] >= 0


def test_play_prints_the_stride_report(tmp_path, monkeypatch, capsys):
    """play() ends with the stride table when the task's config has the switch on, and prints nothing
    of it when it is off."""
    _need_gpu()
    import sys
    import humanoid.scripts.play as play_mod
    from humanoid.envs import XBotLCfg, XBotLCfgPPO  # noqa: F401  (registers humanoid_ppo)
    from humanoid.utils import get_args, task_registry
    tr_mod = sys.modules["humanoid.utils.task_registry"]
    monkeypatch.setattr(tr_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.setattr(play_mod, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    args = get_args(["--num_envs", "64", "--headless", "--run_name", "p"])
    env, _ = task_registry.make_env("humanoid_ppo", args=args)
    _, tcfg = task_registry.get_cfgs("humanoid_ppo")
    tcfg.runner.num_steps_per_env = 8
    runner, tcfg = task_registry.make_alg_runner(env, args=args, train_cfg=tcfg)
    runner.learn(1, init_at_random_ep_len=True)
    del runner, env
    torch.cuda.synchronize()
    capsys.readouterr()
    play_mod.play(get_args(["--task", "humanoid_ppo", "--headless"]), steps=5)
    off = capsys.readouterr().out
    assert "Stride statistics" not in off and "mean_clearance" not in off
    monkeypatch.setattr(XBotLCfg.metrics, "gait", True)
    monkeypatch.setattr(XBotLCfg.metrics, "strides", True)
    play_mod.play(get_args(["--task", "humanoid_ppo", "--headless"]), steps=5)
    on = capsys.readouterr().out
    assert "Gait metrics over the completed episodes:" in on and "Stride statistics over the completed episodes:" in on
    tail = on[on.index("Stride statistics over the completed episodes:"):].splitlines()
    assert tail[1].split() == ["overall", "left", "right", "both"] and tail[2].split()[0] == "strides"
