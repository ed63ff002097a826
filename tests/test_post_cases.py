"""The planted table of oracle/post_cases.py, on the oracle alone (no GPU).

tests/test_gpu_reward_terms.py holds k_post_step to this table; here the table itself is held to
what it promises, so the GPU test cannot pass on rows that miss their branch:

  coverage   every branch of the reward terms, the termination and the heading command is taken on
             both sides by at least 2 rows (rows that do not reset, except for the termination
             itself); every compared quantity keeps its margin to its threshold; at least 95 % of
             the rows are neither excluded (commands redrawn) nor within a margin
  bounds     the float32 oracle lies inside every derived bound of the float64 oracle on every
             row (so no bound is tighter than float32 allows), and is its own bitwise reference
             for the five terms that replay exact selections
  mutants    twelve one-line wrong variants of the oracle (the source text of envlogic_ref.py /
             pipeline_ref.py with one replacement, executed as a module of its own) each break a
             check of post_cases.check on the planted rows

One listed variant is equivalent at float32 and is not among the twelve: without the upper clamp of
the distance terms, exp(-100 x 0.5) becomes exp(-100 (d - max)) for d > max + 0.5, both below
2e-22 next to the other exponential's 0.5 (d > max implies d > min): no float32 sum can tell them
apart.  The planted rows beyond max + 0.5 still pin that the term stays 0.5 there.
"""
import copy
import os
import types

import numpy as np
import pytest

import envlogic_ref as E
import pipeline_ref as PR
import post_cases as PC

ORACLE = os.path.dirname(os.path.abspath(PR.__file__))


def cpu_cfg(n=PC.N):
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    _, js = N.load_model(armature=cfg.sim.hg.armature)
    hc, _ = build_hg_cfg(cfg, n, cfg.sim.dt, 5, js)
    return PR.Cfg(hc)


@pytest.fixture(scope="module")
def planted():
    cfg = cpu_cfg()
    n = PC.N
    r = np.random.RandomState(3)
    S, obs, priv = PR.initial_state(cfg, np.zeros((n, 3), np.float32), 25.0 + 10.0 * r.rand(n), 0.1 + 1.9 * r.rand(n))
    A, tb = PC.plant(S, cfg)
    ref = PC.reference(A, obs, priv, cfg)
    return cfg, A, tb, ref, obs, priv


def _oracle_outputs(ref):
    return PC.collect(ref["S32"], ref["obs"], ref["priv"], ref["rew"], ref["reset"], ref["timeout"])


def test_table_shape_and_counters(planted):
    cfg, A, tb, ref, _, _ = planted
    n = PC.N
    assert 64 < n and n % 16 != 0 and (n + 15) // 16 > 8
    assert PC.COUNTER % int(cfg.c.push_interval) != 0 and cfg.c.push_robots
    ep1 = A["episode_length_buf"].astype(np.int64) + 1
    on = np.nonzero(ep1 % int(cfg.c.resample_interval) == 0)[0]
    assert set(on) == set(tb.idx("resample")) | {i for i in tb.idx("timeout") if ep1[i] == cfg.P.max_episode_length}
    # two resample rows that stay and one that resets; episode sums planted on exactly the resetting rows
    rs = tb.idx("resample")
    assert (~ref["reset"][rs]).sum() == 2 and ref["reset"][rs].sum() == 1
    planted_sums = np.stack([A["episode_sums"][nm] for nm in PC.NAMES])
    assert (planted_sums[:, ~ref["reset"]] == 0).all() and (planted_sums[:, ref["reset"]] != 0).all()
    # the time-out rows: max - 2 and max - 1 stay, max resets; one row times out with base contact
    to = tb.idx("timeout")
    stored = A["episode_length_buf"][to]
    mx = int(cfg.P.max_episode_length)
    assert not ref["reset"][to][stored < mx].any() and ref["reset"][to][stored == mx].all() and set(stored) == {mx - 2, mx - 1, mx}
    bn = np.linalg.norm(A["contact_forces"][:, 0], axis=1)
    assert (ref["timeout"] & (bn > 1)).sum() >= 1 and (ref["timeout"] & (bn > 0.1) & (bn < 1)).sum() >= 1
    assert (np.count_nonzero(A["contact_forces"][bn > 0, 0], axis=1) == 3).all()
    # the gait rows cover a cycle in steps of at most 4, with the window's edges
    g = np.sort(ep1[tb.idx("gait")])
    assert {1, 2, 31, 32, 33, 63} <= set(g) and np.diff(np.concatenate([g, [g[0] + 64]])).max() <= 4
    _, _, st = E.gait(ep1, cfg.P)
    for rows in (ref["reset"], ~ref["reset"]):
        kinds = {tuple(x) for x in st[rows]}
        assert kinds == {(1.0, 0.0), (0.0, 1.0), (1.0, 1.0)}


def test_every_branch_both_sides_and_margins(planted):
    cfg, A, tb, ref, _, _ = planted
    Br, Mg = PC.branches(A, ref, tb, cfg)
    keep = ~ref["reset"]
    assert len(Br) >= 50
    for name, b, reset_allowed in Br:
        b = np.asarray(b, bool)
        if len(b) == PC.N and not reset_allowed:
            b = b[keep]
        assert b.sum() >= 2 and (~b).sum() >= 2, (name, int(b.sum()), int((~b).sum()))
    near = np.zeros(PC.N, bool)
    for name, q, thr, rel in Mg:
        d = np.abs(np.asarray(q, np.float64) - thr).reshape(PC.N, -1)
        assert (d >= rel * abs(thr)).all() and (d > 0).all(), (name, np.nonzero((d < rel * abs(thr)).any(1))[0], d.min())
        near |= (d < rel * abs(thr)).any(1)
    excluded = np.isin(np.arange(PC.N), tb.resample)
    usable = ~(near | excluded)
    assert usable.mean() >= 0.95, usable.mean()
    # the total: at least 4 rows clearly negative (10 x the total's bound), some of them resetting
    # with collision, and at least 4 clearly positive
    raw, tbnd = ref["raw_total64"], ref["total_bound"]
    neg, pos = raw < -10 * tbnd, raw > 10 * tbnd
    assert (neg & ~excluded).sum() >= 4 and (pos & ~excluded).sum() >= 4 and (neg | pos).all()
    assert (neg & ref["reset"]).sum() >= 4 and (neg & ~ref["reset"]).sum() >= 2
    assert (ref["rew"][neg] == 0).all() and (ref["rew"][pos] > 0).all()
    # every planted clip entry has a partner inside, in both tables
    assert {t for _, t, _, _ in tb.clip} == {"o", "p"} == {t for _, t, _ in tb.inside}
    assert {s for _, _, _, s in tb.clip} == {1.0, -1.0}
    cols = lambda t, src: {c for e in src if e[1] == t for c in [e[2]]}  # noqa: E731
    for lo, hi in ((5, 17), (17, 29), (29, 41), (41, 44)):       # dof_pos, dof_vel, actions, angular velocity
        assert any(lo <= c < hi for c in cols("o", tb.clip)) and any(lo <= c < hi for c in cols("o", tb.inside)), (lo, hi)
    for lo, hi in ((5, 17), (17, 29), (29, 41), (41, 53), (53, 56), (56, 59), (62, 64), (64, 67), (67, 68), (68, 69)):
        assert any(lo <= c < hi for c in cols("p", tb.clip)) and any(lo <= c < hi for c in cols("p", tb.inside)), (lo, hi)


def test_float32_oracle_lies_inside_every_bound(planted):
    cfg, A, tb, ref, _, _ = planted
    bad, worst = PC.check(_oracle_outputs(ref), ref, tb, cfg)
    assert bad == [], bad
    assert set(worst) == set(PC.NAMES) - set(PC.DISCRETE) | {"total", "commands[2]"}
    assert max(worst.values()) <= 1.0
    # no bound below one rounding of the increment itself
    keep = ~ref["reset"]
    for nm in PC.NAMES:
        if nm not in PC.DISCRETE:
            assert (ref["bound"][nm][keep] >= PC.U * np.abs(ref["inc64"][nm][keep])).all(), nm
    # the float64 terms took the float32 branches: the discrete terms agree exactly
    for nm in PC.DISCRETE:
        rows = keep & ~np.isin(np.arange(PC.N), tb.resample)
        np.testing.assert_array_equal(ref["terms64"][nm][rows].astype(np.float32), ref["terms32"][nm][rows], err_msg=nm)
    print("float32 oracle |f32 - f64| / bound:", {k: round(v, 3) for k, v in worst.items()})


def test_dtype_argument_sets_the_precision_of_terms_and_sums(planted):
    cfg, A, _, ref, _, _ = planted
    D = copy.deepcopy(ref["D"])
    t = E.rewards({k: (np.asarray(v, np.float32) if getattr(v, "dtype", None) == np.float64 else v) for k, v in D.items()}, cfg.L, cfg.P)
    assert all(v.dtype == np.float32 for v in t.values())
    t64 = E.rewards(copy.deepcopy(D), cfg.L, cfg.P, np.float64)
    assert all(v.dtype == np.float64 for v in t64.values())
    sums = {nm: np.zeros(PC.N, np.float32) for nm in PC.NAMES}
    assert E.total_reward(t, cfg.scales, sums, cfg.P).dtype == np.float32 and all(v.dtype == np.float32 for v in sums.values())


# ------------------------------------------------------------------------------------------ mutants
def _mutated(e_edits=(), p_edits=()):
    """pipeline_ref with the given (old, new) source replacements applied to envlogic_ref.py and
    pipeline_ref.py, each old text occurring exactly once; the real modules stay untouched."""
    def load(fname, edits, inject):
        with open(os.path.join(ORACLE, fname)) as f:
            src = f.read()
        for old, new in edits:
            assert src.count(old) == 1, (fname, old, src.count(old))
            src = src.replace(old, new)
        mod = types.ModuleType(fname[:-3] + "_mutant")
        mod.__dict__.update(inject)
        exec(compile(src, fname, "exec"), mod.__dict__)
        return mod
    Em = load("envlogic_ref.py", e_edits, {})
    return load("pipeline_ref.py", tuple(p_edits) + (("import envlogic_ref as E\n", ""),), {"E": Em})


MUTANTS = {
    "ep >= max_episode_length": dict(e=[("timeout = ep_len > P.max_episode_length", "timeout = ep_len >= P.max_episode_length")]),
    "1.0 and 0.1 swapped in termination and collision": dict(e=[
        ("reset = np.linalg.norm(contact_forces[:, L.base, :], axis=-1) > 1.0", "reset = np.linalg.norm(contact_forces[:, L.base, :], axis=-1) > 0.1"),
        ("(np.linalg.norm(cf32[:, [L.base], :], axis=-1) > 0.1)", "(np.linalg.norm(cf32[:, [L.base], :], axis=-1) > 1.0)")]),
    "contact from the force norm": dict(e=[("    contact = cf32[:, fe, 2] > 5.0\n", "    contact = np.linalg.norm(cf32[:, fe, :], axis=-1) > 5.0\n")]),
    "feet swapped in foot_slip": dict(e=[("axis=2)) * contact, 1)", "axis=2)) * contact[:, ::-1], 1)")]),
    "the 400 clip dropped": dict(e=[("f32(P.max_contact_force), 0, 400), 1)", "f32(P.max_contact_force), 0, np.inf), 1)")]),
    "stance unweighted in base_height": dict(e=[("mh = np.sum(rs[:, fe, 2] * stance, 1) / np.sum(stance, 1)", "mh = np.sum(rs[:, fe, 2], 1) / 2")]),
    "the |sin| < 0.1 window dropped": dict(e=[("    st[np.abs(s) < 0.1] = 1\n", "")]),
    "low_speed's 1.2 as 1.0": dict(e=[("sp > 1.2 * cm", "sp > 1.0 * cm")]),
    "the |cmd| > 0.1 gate dropped": dict(e=[("r * (np.abs(cmd32[:, 0]) > 0.1)", "r * (np.abs(cmd32[:, 0]) > -1.0)")]),
    "max_dist for the knees": dict(e=[("dist_rew(rs[:, kn, :2], P.max_dist / 2)", "dist_rew(rs[:, kn, :2], P.max_dist)")]),
    "no clip on the total": dict(e=[("        rew = np.maximum(rew, 0)\n", "        rew = rew\n")]),
    "no observation clip on dof_vel": dict(p=[("    o, p = np.clip(o, -clip, clip), np.clip(p, -clip, clip)\n",
                                                "    o, p = np.where((np.arange(o.shape[1]) >= 17) & (np.arange(o.shape[1]) < 29), o, np.clip(o, -clip, clip)), np.clip(p, -clip, clip)\n")]),
}
EXPECT = {   # a word that must occur in the violations: the mutant is caught where it is wrong
    "ep >= max_episode_length": "reset_buf", "1.0 and 0.1 swapped in termination and collision": "collision",
    "contact from the force norm": "last_contacts", "feet swapped in foot_slip": "foot_slip", "the 400 clip dropped": "feet_contact_forces",
    "stance unweighted in base_height": "base_height", "the |sin| < 0.1 window dropped": "stance", "low_speed's 1.2 as 1.0": "low_speed",
    "the |cmd| > 0.1 gate dropped": "low_speed", "max_dist for the knees": "knee_distance", "no clip on the total": "rew_buf",
    "no observation clip on dof_vel": "frame o",
}


def test_the_mutant_loader_reproduces_the_oracle(planted):
    cfg, A, tb, ref, obs, priv = planted
    mref = PC.reference(A, obs, priv, cfg, pipeline=_mutated())
    bad, _ = PC.check(_oracle_outputs(mref), ref, tb, cfg)
    assert bad == []
    np.testing.assert_array_equal(mref["rew"], ref["rew"])


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_wrong_oracle_is_caught(planted, name):
    cfg, A, tb, ref, obs, priv = planted
    m = MUTANTS[name]
    mref = PC.reference(A, obs, priv, cfg, pipeline=_mutated(m.get("e", ()), m.get("p", ())))
    bad, _ = PC.check(_oracle_outputs(mref), ref, tb, cfg)
    assert bad and any(EXPECT[name] in b for b in bad), (name, bad)


def test_there_are_twelve_mutants():
    assert len(MUTANTS) >= 12 and set(MUTANTS) == set(EXPECT)
