"""The planted tables of oracle/step_cases.py, on the oracle alone (no GPU).

tests/test_gpu_step_cases.py holds k_step to these tables; here the tables are held to what they
promise, so the GPU test cannot pass on rows that miss their branch:

  coverage    every branch of step_cases.COVER is taken by a row of the table, by the oracle's own
              detection (physics_ref.c ref_detect) and the row budget that follows from it; every row
              takes the branches it is listed for; the layout (planted rows next to flight rows, odd
              count, every warm-start slot planted)
  margins     every decision of every row keeps its stated floor in float64
  budget      the Python restatement of the row budget is pinned to ref_step: equal dropped counts,
              every slot it clears is exactly 0 after the step, every non-zero slot is one it keeps
  f32 = f64   the f32 oracle takes the same branch code and activity on every item of every row,
              drops the same rows and clears the same slots
  yardstick   the f32 oracle, its kernel-quotient variant and four perturbed f32 builds judged against
              a yardstick that excludes them have ZERO rows outside K = 12 on all seven fields at one
              substep (a condition on the table, not an allowance), which also measures the new
              fields' multiples
  mutants     sixteen one-line wrong variants of physics_ref.c (the source with one replacement,
              compiled under oracle/_ref/) each break a check the GPU test makes, on the table named

No variant on the list is equivalent on the tables.  One was at first: without the near-parallel
case, exactly parallel thigh axes still end with s = 0 (the quotient's sign is rounding noise, and
the t clamp's own formula for s is shared), so the row thighs_near_parallel was added — axes 2e-4 rad
apart, converging towards the far ends, where the missing case moves the contact point by the
length of the thigh.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import physics_ref as P
import step_cases as SC
import step_tolerance as ST

ORACLE = os.path.dirname(os.path.abspath(P.__file__))
KINDS = ("plane", "heightfield", "fixed")
SEED = 5   # the run seed of the GPU test's envs: the heightfield generator's


def cpu_cfg(kind, decimation=1):
    """hg_cfg, model and height samples of the env the GPU test makes for `kind`."""
    from humanoid import _native as N
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    cfg = XBotLCfg()
    cfg.control.decimation = decimation
    hf, ptr, shape = None, None, (0, 0)
    if kind == "heightfield":
        from humanoid.utils.terrain import HumanoidTerrain
        cfg.terrain.mesh_type = "heightfield"
        saved = np.random.get_state()
        np.random.seed(SEED)   # as XBotLFreeEnv.create_sim seeds the generator
        try:
            hf = np.ascontiguousarray(HumanoidTerrain(cfg.terrain, 64).heightsamples, np.int16)
        finally:
            np.random.set_state(saved)
        ptr, shape = hf.ctypes.data, hf.shape
    cfg.asset.fix_base_link = kind == "fixed"
    model, js = N.load_model(armature=cfg.sim.hg.armature)
    hc, _ = build_hg_cfg(cfg, 8, cfg.sim.dt, 5, js, ptr, shape)
    return hc, model, hf


@pytest.fixture(scope="module")
def refs():
    out = {}
    for kind in KINDS:
        hc, model, hf = cpu_cfg(kind)
        tb = SC.table(kind, hc, model, hf)
        out[kind] = SC.Reference(tb, hc, model, hf)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_layout(refs, kind):
    R = refs[kind]
    tb = R.tb
    assert tb.n % 2 == 1 and tb.n == SC.SIZES[kind]
    assert (tb.lam != 0).all()
    assert not R.r64.nonfinite.any()
    if kind != "fixed":
        # every planted row sits next to a flight row without contacts
        flight = np.array([n.startswith("flight") for n in tb.names])
        assert flight[1::2].all() and not flight[0::2].any()
        assert not (R.D["active"][flight] == 1).any()
        w = np.linalg.norm(tb.root_states[flight, 10:13], axis=1)
        assert w.min() >= 4.9 and w.max() >= 19.9 and (tb.root_states[flight, 2] > 2.8).all()
        R0 = tb.root_states[flight, 3:7]
        assert (np.abs(R0).min(axis=0) < 0.2).all() and (np.abs(R0).max(axis=0) > 0.8).all()   # all over the sphere


@pytest.mark.parametrize("kind", KINDS)
def test_every_branch_is_taken(refs, kind):
    R = refs[kind]
    B = SC.branches(R.tb, R.hc, R.model, R.D, R.PL)
    taken = set().union(*B)
    assert [b for b in SC.COVER[kind] if b not in taken] == []
    for e, want in enumerate(R.tb.targets):
        assert [t for t in want if t not in B[e]] == [], (e, R.tb.names[e])
    if kind == "plane":
        # the issue's three fallen poses: more than nine active candidates, round-2 items among the kept
        fd = R.tb.names.index("face_down_yaw0")
        act = np.flatnonzero(R.D["active"][fd])
        assert len(act) == 12 and R.PL["dropped"][fd] == 9 and (act >= 32).sum() == 4
        assert np.flatnonzero(R.PL["kept"][fd])[-1] == 33   # ground candidate 20 takes the ninth slot
        assert R.PL["dropped"][R.tb.names.index("on_side0")] == 3
        assert R.PL["dropped"][R.tb.names.index("squat_yaw0")] >= 12
        six = R.tb.names.index("face_down_six_limits")
        assert R.PL["nrows"][six] == 32 and (R.PL["lim_on"][six] & ~R.PL["lim_kept"][six]).sum() >= 1


@pytest.mark.parametrize("kind", KINDS)
def test_margins_hold(refs, kind):
    R = refs[kind]
    assert SC.margin_failures(R.tb, R.hc, R.model, R.D) == []


@pytest.mark.parametrize("kind", KINDS)
def test_budget_restatement_is_pinned_to_ref_step(refs, kind):
    R = refs[kind]
    np.testing.assert_array_equal(R.PL["dropped"], R.r64.dropped)
    assert (R.r64.lam[R.PL["cleared"]] == 0).all()
    assert (~R.PL["cleared"][R.r64.lam != 0]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_f32_oracle_takes_the_f64_branches(refs, kind):
    R = refs[kind]
    D32 = SC.detect(R.tb, R.hc, R.model, R.hf, "f32")
    np.testing.assert_array_equal(D32["code"], R.D["code"])
    np.testing.assert_array_equal(D32["active"], R.D["active"])
    out, dropped = R.run("f32")
    np.testing.assert_array_equal(dropped, R.r64.dropped)
    np.testing.assert_array_equal(out["lam"] == 0, R.r64.lam == 0)


@pytest.mark.parametrize("kind", KINDS)
def test_f32_builds_have_no_outliers_at_one_substep(refs, kind):
    """The issue's condition on the table: the f32 oracle through check_step on all seven fields,
    zero outlier envs.  That build is a member of the yardstick's own ensemble, so the same is
    required of builds that are not: the kernel-quotient f32 variant and four perturbed f32
    members judged against the first three."""
    R = refs[kind]
    out, _ = R.run("f32")
    _, rep, fails, _ = ST.check_step(R.hc, R.model, R.S, R.a, out, SC.FIELDS7, R.hf)
    assert not fails and rep["outlier_envs"] == 0, (fails, rep)
    worst = {f: 0.0 for f in SC.FIELDS7}
    cands = ST.f32_members(R.hc, R.model, R.S, R.a, SC.FIELDS7, R.hf, members=4, first=3)
    outq, dq = R.run("f32q")
    for c, d in [(c, c["dropped"]) for c in cands] + [(outq, dq)]:
        v, head = R.violations(c, d)
        assert v == []
        worst = {f: max(worst[f], head[f]) for f in SC.FIELDS7}
    print(kind, "largest multiple of the yardstick over the independent f32 builds:", {f: round(v, 2) for f, v in worst.items()})
    # K = 12 (STEP_TOL_K) fits the two new fields: no independent f32 build exceeds it
    assert worst["contact"] < ST.STEP_TOL_K and worst["lam"] < ST.STEP_TOL_K


# (table on which it must fail, the line of physics_ref.c, its wrong form)
MUTANTS = {
    "seg_seg t > 1 clamp uses the t < 0 formula": (
        "plane", "else if (t > 1) { t = 1; s = clamp01(QDIV(b - c, a)); code |= DS_THI; }",
        "else if (t > 1) { t = 1; s = clamp01(QDIV(-c, a)); code |= DS_THI; }"),
    "seg_seg never takes the near-parallel case": (
        "plane", "  real s = denom > R(1e-6) * a * e ? clamp01(QDIV(b * f - c * e, denom)) : 0;",
        "  real s = clamp01(QDIV(b * f - c * e, denom));"),
    "tangent reference always x": ("plane", "ref[fabs(n[0]) < R(0.9) ? 0 : 1] = 1;", "ref[0] = 1;"),
    "eight contact points instead of nine": ("plane", "#define MAX_CONTACT_POINTS 9", "#define MAX_CONTACT_POINTS 8"),
    "a dropped limit row's slot is not cleared": (
        "plane", "if (nr >= MAX_ROWS) { lamst[LAM_LIM + j] = 0; *dropped += 1; continue; }",
        "if (nr >= MAX_ROWS) { *dropped += 1; continue; }"),
    "damping kept when the torque is saturated": ("plane", "madd[j] = sat ? 0 : dt * R(cfg->kd[j]);", "madd[j] = dt * R(cfg->kd[j]);"),
    "no vmax cap on contact rows": (
        "plane", "r->target = ct->phi >= 0 ? -ct->phi / dt : fmin(-beta * ct->phi / dt, vmax);",
        "r->target = ct->phi >= 0 ? -ct->phi / dt : -beta * ct->phi / dt;"),
    "no vmax cap on limit rows": (
        "plane", "r->target = gap >= 0 ? -gap / dt : fmin(-beta * gap / dt, vmax);", "r->target = gap >= 0 ? -gap / dt : -beta * gap / dt;"),
    "speculative contacts get the Baumgarte target": (
        "plane", "r->target = ct->phi >= 0 ? -ct->phi / dt : fmin(-beta * ct->phi / dt, vmax);",
        "r->target = fmin(-beta * ct->phi / dt, vmax);"),
    "upper-triangle gradient taken from the lower triangle": (
        "heightfield", "dhdx = (h11 - h01) / hs; dhdy = (h01 - h00) / hs; }", "dhdx = (h10 - h00) / hs; dhdy = (h11 - h10) / hs; }"),
    "pair friction coefficient from the ground formula": (
        "fixed", "      ct->mu = fric;", "      ct->mu = R(0.5) * (fric + cfg->ground_friction);"),
    "-lambda d on bN with the wrong sign in the contact force": (
        "fixed", "if (rr->bneg >= 0) cf_out[rr->bneg * 3 + i] -= f;", "if (rr->bneg >= 0) cf_out[rr->bneg * 3 + i] += f;"),
    "upper joint limit pushes the wrong way": (
        "fixed", "else if (ghi < lim_margin) { sgn = -1; gap = ghi; }", "else if (ghi < lim_margin) { sgn = 1; gap = ghi; }"),
    "box face ignores its rectangle": ("plane", "dist = inside ? h[s] : R(1e3);", "dist = h[s];"),
    "box face tests the farther end sphere": ("fixed", "const int s = h[1] < h[0] ? 1 : 0;", "const int s = h[1] > h[0] ? 1 : 0;"),
    "quaternion integrated with the full angle": (
        "plane", "real s = sin(th / 2) / (th / dt), c = cos(th / 2);", "real s = sin(th) / (th / dt), c = cos(th);"),
}


@pytest.fixture(scope="module")
def mutant_dir():
    d = os.path.join(ORACLE, "_ref")
    os.makedirs(d, exist_ok=True)
    return d


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_wrong_oracle_fails_on_the_table(refs, mutant_dir, name):
    kind, old, new = MUTANTS[name]
    with open(os.path.join(ORACLE, "physics_ref.c")) as f:
        src = f.read()
    assert src.count(old) == 1, "the mutated line is not unique in physics_ref.c"
    tag = "mutant_" + "".join(ch if ch.isalnum() else "_" for ch in name)[:48]
    c_path, so_path = os.path.join(mutant_dir, tag + ".c"), os.path.join(mutant_dir, tag + ".so")
    with open(c_path, "w") as f:
        f.write(src.replace(old, new).replace('#include "../include/hgsim.h"', '#include "../../include/hgsim.h"'))
    subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-std=gnu11", "-o", so_path, c_path, "-lm"], check=True)
    R = refs[kind]
    out, dropped = R.run("f64", library=ctypes.CDLL(so_path))
    v, _ = R.violations(out, dropped)
    print(name, "->", v[:4])
    assert v, f"the wrong oracle ({name}) passes every check on the {kind} table"
    # and the unmodified source, built the same way, passes: the failure is the replacement's
    if name == sorted(MUTANTS)[0]:
        with open(c_path, "w") as f:
            f.write(src.replace('#include "../include/hgsim.h"', '#include "../../include/hgsim.h"'))
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", "-std=gnu11", "-o", so_path + ".orig", c_path, "-lm"], check=True)
        out, dropped = R.run("f64", library=ctypes.CDLL(so_path + ".orig"))
        assert R.violations(out, dropped)[0] == []


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_ref_step_is_bit_identical_to_before_detect_was_factored_out(precision):
    """physics_ref.c's detection loop became detect() (shared with ref_detect) and reports branch
    codes; ref_step's outputs on the recorded state of tests/golden/kstep_outlier_r6.npz are bit for
    bit those of the source before that change (tests/golden/ref_step_parent_r6.npz)."""
    import sys
    repo = os.path.dirname(ORACLE)
    sys.path.insert(0, os.path.join(repo, "scripts"))
    import classify_kstep_outlier as C
    D = np.load(os.path.join(repo, "tests", "golden", "kstep_outlier_r6.npz"), allow_pickle=False)
    G = np.load(os.path.join(repo, "tests", "golden", "ref_step_parent_r6.npz"), allow_pickle=False)
    S = {k[2:]: D[k] for k in D.files if k.startswith("S_")}
    hc, model, _ = C.smoke_cfg(D["a_ref"].shape[0])
    sim = ST.ref_sim(hc, model, S, precision)
    sim.step(D["a_ref"])
    for k in ("q", "qd", "root", "torques", "rigid", "contact", "lam", "dropped", "nonfinite"):
        assert getattr(sim, k).tobytes() == G[f"{precision}_{k}"].tobytes(), k
