"""k_step on the planted tables of oracle/step_cases.py against the f64 C reference physics.

Each table (plane, heightfield, fixed base) is written through the env's views — root, joints,
previous actions, warm-start impulses, base mass and friction — into an env of the table's own size,
and ONE hg_step is launched on it.  tests/test_step_cases.py shows on the oracle alone that every row
takes the branch it is there for, at a margin no fp32 build can cross, and that independent f32
builds have no row outside the tolerance at one substep; so here, with control.decimation = 1:

  * oracle/step_tolerance.check_step on all seven fields — q, qd, root, torques, rigid states and
    the two no other test compares, the contact forces and the warm-start impulses — with ZERO
    outlier envs at the shared K = 12;
  * rows dropped over the budget equal the oracle's env for env; every warm-start slot the oracle's
    detection clears is exactly 0; the non-finite counter is untouched;
  * with HG_WAVE_BALANCE 0 (envs 2k and 2k + 1 in one wave: every fallen row next to a flight row)
    and 1 (the env order the product's own post launch sorted from the rows of a priming step on
    the same table) every field is bit for bit the same.

The same tables once more at the product's decimation = 10, under check_step's rule as it stands
(outliers held to the fp32 null rate), dropped counts compared on the rows where every CPU f32
build agrees with f64.
"""
import ctypes

import numpy as np
import pytest
import torch

import step_cases as SC
import step_tolerance as ST
from test_gpu_parity import _make_env, _need_gpu, _hf

pytestmark = pytest.mark.gpu

OVERRIDES = {"plane": {}, "heightfield": {"terrain__mesh_type": "heightfield"}, "fixed": {"asset__fix_base_link": True}}
OUT = ("dof_pos", "dof_vel", "root_states", "torques", "rigid_state", "contact_forces", "rows_dropped", "nonfinite_count")
COUNTER = 4242


def _plant(env, tb, root=None):
    from humanoid import _native as N
    dev = env.root_states.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    env.root_states[:] = t(tb.root_states if root is None else root)
    env.dof_pos[:] = t(tb.dof_pos)
    env.dof_vel[:] = t(tb.dof_vel)
    env.actions[:] = t(tb.actions)          # the previous actions: the delay blend of equal actions is the action
    env._view(N.T["CONTACT_LAMBDA"])[:] = t(tb.lam)
    env.body_mass[:] = t(tb.body_mass)
    env.env_frictions[:] = t(tb.env_frictions)
    torch.cuda.synchronize()


def _run(kind, decimation, balance, monkeypatch):
    """Plant the table in a fresh env and launch one hg_step on it.  Returns (env, table, a_ref,
    outputs as numpy, the env order the step ran with)."""
    from humanoid import _native as N
    import pipeline_ref as PR
    monkeypatch.setenv("HG_WAVE_BALANCE", balance)
    n = SC.SIZES[kind]
    env = _make_env(n, control__decimation=decimation, **OVERRIDES[kind])
    hc, model, hf = env._hgcfg, env._model, _hf(env)
    tb = SC.table(kind, hc, model, hf)
    assert tb.n == n
    # priming: one product step (hg_step + hg_post) on the table, so that the post launch sorts the
    # env order from this table's own row counts; the rows outside the heightfield's edges fly over
    # its middle meanwhile (the post launch is not asked to handle positions off the map)
    safe = tb.root_states.copy()
    for e, name in enumerate(tb.names):
        if name.startswith("edge_"):
            safe[e, 0:3] = (30.0, 30.0, 3.0)
    _plant(env, tb, safe)
    env.step(torch.zeros(n, 12, device="cuda:0"))
    torch.cuda.synchronize()
    _plant(env, tb)
    g = lambda x: x.detach().cpu().numpy().copy()  # noqa: E731
    before = {k: g(getattr(env, k)) for k in ("rows_dropped", "nonfinite_count")}
    act = torch.from_numpy(tb.actions).to("cuda:0")
    a_ref = PR.preprocess_actions(PR.Cfg(hc), tb.actions, tb.actions, COUNTER)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(N.lib().hg_step(env.sim, ctypes.c_void_p(act.data_ptr()), ctypes.c_uint64(COUNTER), s), env.sim)
    torch.cuda.synchronize()
    np.testing.assert_allclose(g(env.actions), a_ref, rtol=1e-5, atol=1e-6)
    out = {k: g(getattr(env, k)) for k in OUT}
    out["lam"] = g(env._view(N.T["CONTACT_LAMBDA"]))
    out["rows_dropped"] -= before["rows_dropped"]
    out["nonfinite_count"] -= before["nonfinite_count"]
    return env, tb, a_ref, out, g(env.env_order)


def _both(kind, decimation, monkeypatch):
    env, tb, a_ref, out0, _ = _run(kind, decimation, "0", monkeypatch)
    _, _, a1, out1, order = _run(kind, decimation, "1", monkeypatch)
    np.testing.assert_array_equal(a_ref, a1)
    assert (order != np.arange(tb.n)).any(), "the balanced run kept the identity order: the sort was not exercised"
    for k in out0:
        np.testing.assert_array_equal(out0[k], out1[k], err_msg=f"{k}: HG_WAVE_BALANCE 0 and 1 differ")
    cand = {"q": out0["dof_pos"], "qd": out0["dof_vel"], "root": out0["root_states"], "torques": out0["torques"],
            "rigid": out0["rigid_state"], "contact": out0["contact_forces"], "lam": out0["lam"]}
    return env, tb, a_ref, cand, out0


@pytest.mark.parametrize("kind", ["plane", "heightfield", "fixed"])
def test_planted_substep_matches_the_oracle(kind, monkeypatch):
    _need_gpu()
    env, tb, a_ref, cand, out = _both(kind, 1, monkeypatch)
    hc, model, hf = env._hgcfg, env._model, _hf(env)
    D = SC.detect(tb, hc, model, hf)
    PL = SC.plan(tb, hc, model, D)
    # the table as this env sees it (its own height samples, the preprocessed actions) keeps its promises
    assert SC.margin_failures(tb, hc, model, D, actions=a_ref) == []
    taken = set().union(*SC.branches(tb, hc, model, D, PL))
    assert [b for b in SC.COVER[kind] if b not in taken] == []
    r64, report, fails, bad = ST.check_step(hc, model, tb.state(), a_ref, cand, SC.FIELDS7, hf)
    print(kind, "achieved multiples of the yardstick:", {f: round(v, 2) for f, v in report["ratio"].items()})
    names = [tb.names[i] for i in report["outlier_ids"]]
    assert not fails and report["outlier_envs"] == 0, (names, {f: np.argwhere(bad[f])[:6].tolist() for f in bad if bad[f].any()}, fails)
    assert not r64.nonfinite.any() and not out["nonfinite_count"].any()
    np.testing.assert_array_equal(out["rows_dropped"], r64.dropped)
    np.testing.assert_array_equal(r64.dropped, PL["dropped"])
    kept_nonzero = (cand["lam"] != 0) & PL["cleared"]
    assert not kept_nonzero.any(), [(tb.names[e], np.flatnonzero(kept_nonzero[e]).tolist()) for e in np.flatnonzero(kept_nonzero.any(1))]


@pytest.mark.parametrize("kind", ["plane", "heightfield", "fixed"])
def test_planted_step_at_the_product_decimation(kind, monkeypatch):
    """Ten substeps from the planted states: check_step's rule unchanged (outlier envs held to the
    measured f32 null rate).  Rows whose f64 oracle turns non-finite within the step would be left
    out of this run, by name, at most one in ten; none does."""
    _need_gpu()
    env, tb, a_ref, cand, out = _both(kind, 10, monkeypatch)
    hc, model, hf = env._hgcfg, env._model, _hf(env)
    S = tb.state()
    probe = ST.ref_sim(hc, model, S, "f64", hf)
    probe.step(a_ref)
    left_out = [tb.names[e] for e in np.flatnonzero(probe.nonfinite)]
    assert left_out == [], left_out
    r64, report, fails, _ = ST.check_step(hc, model, S, a_ref, cand, SC.FIELDS7, hf)
    print(kind, "achieved multiples of the yardstick:", {f: round(v, 2) for f, v in report["ratio"].items()},
          "outliers", [tb.names[i] for i in report["outlier_ids"]], "allowed", report.get("allowed_outlier_envs", 0))
    assert not fails, " | ".join(fails)
    assert not out["nonfinite_count"].any()
    builds = ST.f32_members(hc, model, S, a_ref, ("q",), hf, members=7)
    agree = np.all([b["dropped"] == r64.dropped for b in builds], axis=0)
    assert agree.mean() >= 0.9
    np.testing.assert_array_equal(out["rows_dropped"][agree], r64.dropped[agree])
