"""Planted states for K_step's contact detection, row budget, targets and forces — TEST INFRASTRUCTURE ONLY.

Shared by tests/test_step_cases.py (CPU: coverage, margins, f32 / f64 agreement, wrong oracles) and
tests/test_gpu_step_cases.py (the kernel), in the manner of oracle/post_cases.py.

  table(kind, hc, model, hf=None)   kind "plane" | "heightfield" | "fixed": a Table of one env per row —
                                    root_states, dof_pos, dof_vel, actions, lambda, body_mass,
                                    env_frictions, a name per row and the branches the row is there for
  detect(tb, hc, model, hf, prec)   the oracle's own detection of the planted substep (physics_ref.c
                                    ref_detect: gap, active flag, normal, branch code and the compared
                                    quantities per item)
  plan(tb, hc, model, D)            the row budget that follows from a detection: kept / over-budget
                                    contact points, kept / dropped limit and friction rows, the warm-start
                                    slots the substep must clear, the dropped count.  Integer logic only
                                    (physics_ref.c substep, "rows"); tests/test_step_cases.py pins it to
                                    ref_step on every row.
  branches(tb, hc, model, D, PL)    the branch names (BRANCHES) each row takes, from D and PL
  margins(tb, hc, model, D)         per row, the least distance of every decision of the substep from its
                                    branch point, by kind (MARGINS gives the floor each kind must keep)

Layout.  Even rows are the planted cases; odd rows are "flight" rows (z = 3 m, a random unit quaternion,
|w| between 5 and 20 rad/s, joint velocities of a few rad/s, no contact).  With wave balancing off envs
2k and 2k + 1 share a wave, so every fallen row runs next to a row without contacts (round 2 of the
detection then runs for a wave in which only one env can have a round-2 contact, and the plane
early-out is taken by the waves whose planted row stands or flies).  The row count is odd: the last
wave is ragged.  Every warm-start slot is planted non-zero (LAM0), so a slot the kernel should clear
but does not shows up.

Margins (MARGINS).  A row is only useful if no fp32 build can take another branch on it, so every
decision keeps a floor that is large against fp32 rounding of the compared quantity:
  phi      |phi - contact_offset|, |phi| and |phi + vmax dt / beta| of every item: 1e-4 m (positions are
           below 64 m: one ulp is 4e-6 m)
  limit    the same three for a joint-limit gap (0.01, 0, -vmax dt / beta): 1e-4 rad
  seg      s and t of every capsule pair within 5 cm of the contact offset from 0 and 1: 1e-3; its
           denom / (a e) is below 1e-7 or above 1e-5 (the test is at 1e-6; fp32 cancellation in
           a e - b b is about 1e-7 a e).  A pair further out places no contact whichever closest
           points it finds (the default pose itself has the two feet parallel to 5e-7); the CPU test
           still requires the f32 oracle to take the f64 code on every item.
  box      |h1 - h0| and the chosen end's distance from the rectangle's edges: 1e-3 m
  nx       ||n.x| - 0.9| of every active contact: 0.05
  tau      ||t_pd| - limit| of every joint: 2 % of the limit + 1 N m (the action noise of the step
           prologue is 2 % of the action, and the planted actions alone never carry more than the limit)
  uv       |u - v| and the distance of (u, v) from the cell's edges, heightfield: 0.02 cells (2 mm)

Not planted, because the state cannot reach them: the coincident-axes fallback of a capsule pair
(dist <= 1e-9: the model's capsules would have to intersect axis on axis, and the gap is then
-(ra + rb), far past every other bound), and the quaternion exponential's th == 0 on a floating
base (gravity alone gives the base a non-zero angular velocity after the solve unless every
coupling vanishes exactly).  The fixed-base table runs the th-free branch (root velocities zeroed).
"""
import numpy as np

import physics_ref as P

NC, NPAIR, ND = 24, 16, 12
LAM_PAIR, LAM_LIM = NC * 3, NC * 3 + NPAIR * 3
LAM_FRIC = LAM_LIM + ND
LAMW = LAM_FRIC + ND
MAX_ROWS, MAX_POINTS = 32, 9
LIM_MARGIN = 0.01

MARGINS = dict(phi=1e-4, limit=1e-4, seg=1e-3, par_lo=1e-7, par_hi=1e-5, box=1e-3, nx=0.05, tau_rel=0.02, tau_abs=1.0,
               uv=0.02)

# warm-start plant: normal, the two tangents (inside every cone: mu >= 0.35), limit, joint friction
# (inside the bound f dt = 1e-4)
LAM0 = dict(n=0.01, t1=0.002, t2=-0.001, lim=0.005, fric=5e-5)

BRANCHES = (
    "round2_runs", "round2_ranks_after_round1", "round2_mixed_wave", "round2_skipped", "over_9_points",
    "limit_row_dropped", "friction_row_dropped", "friction_after_limits",
    "seg_parallel", "seg_t_below_0", "seg_t_above_1", "seg_interior",
    "box_end0", "box_end1", "box_inside", "box_outside",
    "tangent_ref_x", "tangent_ref_y",
    "contact_target_speculative", "contact_target_baumgarte", "contact_target_vmax",
    "limit_lower_approach", "limit_lower_penetrated", "limit_upper_approach", "limit_upper_penetrated", "limit_target_vmax",
    "torque_saturated_pos", "torque_saturated_neg", "torque_unsaturated",
    "hf_lower_triangle", "hf_upper_triangle", "hf_clamp_i_low", "hf_clamp_i_high", "hf_clamp_j_low", "hf_clamp_j_high",
    "flight_any_orientation",
)
# the branches each kind of table must cover (tests/test_step_cases.py)
COVER = {
    "plane": [b for b in BRANCHES if not b.startswith("hf_")],
    "heightfield": ["hf_lower_triangle", "hf_upper_triangle", "hf_clamp_i_low", "hf_clamp_i_high", "hf_clamp_j_low",
                    "hf_clamp_j_high", "round2_runs", "over_9_points", "contact_target_baumgarte"],
    "fixed": ["seg_parallel", "seg_t_below_0", "seg_t_above_1", "box_inside", "tangent_ref_y", "tangent_ref_x",
              "limit_lower_penetrated", "limit_upper_penetrated", "limit_target_vmax", "torque_saturated_pos",
              "torque_saturated_neg", "friction_after_limits"],
}


def quat_rpy(roll, pitch, yaw):
    """(x, y, z, w) of the intrinsic z-y-x rotation, float64."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


class Table:
    def __init__(self, kind):
        self.kind, self.names, self.targets = kind, [], []
        self.root, self.q, self.qd, self.act = [], [], [], []

    def add(self, name, targets, z=3.0, rpy=(0, 0, 0), xy=(0, 0), q=None, qd=None, v=(0, 0, 0), w=(0, 0, 0), act=None,
            quat=None):
        root = np.zeros(13)
        root[0:2], root[2] = xy, z
        root[3:7] = quat_rpy(*rpy) if quat is None else quat
        root[7:10], root[10:13] = v, w
        self.names.append(name)
        self.targets.append(tuple(targets))
        self.root.append(root)
        self.q.append(np.zeros(ND) if q is None else np.asarray(q, np.float64))
        self.qd.append(np.zeros(ND) if qd is None else np.asarray(qd, np.float64))
        self.act.append(np.zeros(ND) if act is None else np.asarray(act, np.float64))

    def finish(self, model, seed):
        """float32 arrays (what the env's views hold), the planted warm start and seeded per-env base
        mass and friction inside the randomisation ranges (the GPU test writes them into the env
        with the rest)."""
        f = lambda x: np.ascontiguousarray(np.array(x, np.float64).astype(np.float32))  # noqa: E731
        self.root_states, self.dof_pos, self.dof_vel, self.actions = f(self.root), f(self.q), f(self.qd), f(self.act)
        self.n = len(self.names)
        lam = np.zeros((self.n, LAMW), np.float32)
        for k, key in enumerate(("n", "t1", "t2")):
            lam[:, k:LAM_LIM:3] = LAM0[key]
        lam[:, LAM_LIM:LAM_FRIC] = LAM0["lim"]
        lam[:, LAM_FRIC:] = LAM0["fric"]
        self.lam = lam
        r = np.random.default_rng(seed)
        self.body_mass = (model.mass[0] + r.uniform(-5, 5, self.n)).astype(np.float32).reshape(-1, 1)
        self.env_frictions = r.uniform(0.1, 2.0, self.n).astype(np.float32).reshape(-1, 1)
        return self

    def state(self):
        """The dict oracle/step_tolerance.py calls S."""
        return {"root_states": self.root_states, "dof_pos": self.dof_pos, "dof_vel": self.dof_vel, "lambda": self.lam,
                "body_mass": self.body_mass, "env_frictions": self.env_frictions}

    def rows(self, target):
        return [i for i, t in enumerate(self.targets) if target in t]


def limits(model):
    return (np.array([model.lower[b] for b in range(1, ND + 1)], np.float64),
            np.array([model.upper[b] for b in range(1, ND + 1)], np.float64))


# ---------------------------------------------------------------------------------------- planted poses
# joint order: left roll, yaw, pitch, knee, ankle pitch, ankle roll, then the right leg
# hips -1.5 rad, knees 1.0 rad; the base at 0.1095 m, not 0.11 m, where the box's lower corners
# (0.1 m below the origin) would sit on the contact offset itself
SQUAT = [0, 0, -1.5, 1.0, 0, 0, 0, 0, -1.5, 1.0, 0, 0]
# capsule-pair poses, found by a seeded search over the joint ranges for the wanted branch code on an
# ACTIVE pair with every item of the pose inside MARGINS (the search is not part of the table; the
# CPU test re-derives code, activity and margins from these literals)
PAIR_POSES = {}


def _flight_rows(tb, count, seed, hc, model):
    """`count` (name, kwargs) rows in flight: z about 3 m, random unit quaternion, |w| in [5, 20] rad/s,
    |v| up to 1 m/s, joints within 0.25 rad of the default pose, joint velocities up to 3 rad/s."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(count):
        qt = r.standard_normal(4)
        qt /= np.linalg.norm(qt)
        w = r.standard_normal(3)
        w *= (5 + 15 * (k % 4) / 3) / np.linalg.norm(w)   # 5, 10, 15, 20 rad/s
        kw = dict(z=3.0 + 0.1 * r.uniform(-1, 1), quat=qt, w=w, v=r.uniform(-1, 1, 3), xy=r.uniform(-1, 1, 2),
                  qd=r.uniform(-3, 3, ND))
        while True:   # joints redrawn until no capsule pair is within 2 cm of the contact offset
            kw["q"] = r.uniform(-0.25, 0.25, ND)
            t = Table("x")
            t.add("x", (), **kw)
            t.finish(model, 0)
            D = detect(t, hc, model)
            if ((D["phi"][0, model.num_leg_contacts:model.num_leg_contacts + model.num_pairs] > hc.contact_offset + 0.02).all()
                    and not margin_failures(t, hc, model, D)):
                break
        out.append((f"flight{k}", kw))
    return out


def _interleave(tb, cases, seed, hc, model):
    fl = _flight_rows(tb, len(cases) - 1, seed, hc, model)
    for k, (name, targets, kw) in enumerate(cases):
        tb.add(name, targets, **kw)
        if k < len(fl):
            tb.add(fl[k][0], ("flight_any_orientation",), **fl[k][1])
    assert len(tb.names) % 2 == 1
    return tb.finish(model, seed)


# ---------------------------------------------------------------------------------------- analysis
def detect(tb, hc, model, hf=None, precision="f64"):
    D = P.detect(hc, model, tb.root_states, tb.dof_pos, tb.body_mass[:, 0], precision, heightfield=hf)
    nit = model.num_contacts + model.num_pairs
    return {k: v[:, :nit] for k, v in D.items()}


def item_slots(model):
    """Warm-start base slot of every detection item (priority order), and whether it is a pair."""
    nleg, npair, nc = model.num_leg_contacts, model.num_pairs, model.num_contacts
    base, pair = [], []
    for item in range(nc + npair):
        is_pair = nleg <= item < nleg + npair
        base.append(LAM_PAIR + 3 * (item - nleg) if is_pair else 3 * (item if item < nleg else item - npair))
        pair.append(is_pair)
    return np.array(base), np.array(pair)


def friction_order(model):
    jf = [model.joint_friction[j + 1] for j in range(ND)]
    return sorted(range(ND), key=lambda j: (-jf[j], j % 6, j)), jf


def limit_gaps(tb, model):
    """(active, sign, gap) of the joint-limit rows: the lower side wins when both are within the margin."""
    lo, hi = limits(model)
    q = tb.dof_pos.astype(np.float64)
    glo, ghi = q - lo, hi - q
    lower, upper = glo < LIM_MARGIN, (glo >= LIM_MARGIN) & (ghi < LIM_MARGIN)
    return lower | upper, np.where(lower, 1.0, -1.0), np.where(lower, glo, ghi)


def plan(tb, hc, model, D):
    n, nit = tb.n, model.num_contacts + model.num_pairs
    base, _ = item_slots(model)
    order, jf = friction_order(model)
    lim_on, _, _ = limit_gaps(tb, model)
    kept = np.zeros((n, nit), bool)
    over = np.zeros((n, nit), bool)
    lim_kept, fric_kept = np.zeros((n, ND), bool), np.zeros((n, ND), bool)
    cleared = np.zeros((n, LAMW), bool)
    dropped, nrows, fric_first = np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    for e in range(n):
        npts = 0
        for it in range(nit):
            if D["active"][e, it] and npts < MAX_POINTS:
                kept[e, it] = True
                npts += 1
            else:
                over[e, it] = bool(D["active"][e, it])
                dropped[e] += 3 * over[e, it]
                cleared[e, base[it]:base[it] + 3] = True
        nr = 3 * npts
        for j in range(ND):
            if lim_on[e, j] and nr < MAX_ROWS:
                lim_kept[e, j] = True
                nr += 1
            else:
                dropped[e] += int(lim_on[e, j])
                cleared[e, LAM_LIM + j] = True
        fric_first[e] = nr
        for j in order:
            if jf[j] > 0 and nr < MAX_ROWS:
                fric_kept[e, j] = True
                nr += 1
            else:
                dropped[e] += int(jf[j] > 0)
                cleared[e, LAM_FRIC + j] = True
        nrows[e] = nr
    return dict(kept=kept, over=over, lim_on=lim_on, lim_kept=lim_kept, fric_kept=fric_kept, cleared=cleared,
                dropped=dropped, nrows=nrows, fric_first=fric_first, npts=kept.sum(1))


def pd_torque(tb, hc, actions=None):
    a = (tb.actions if actions is None else actions).astype(np.float64)
    kp, kd = np.array(hc.kp[:ND]), np.array(hc.kd[:ND])
    dflt, lim = np.array(hc.default_dof_pos[:ND]), np.array(hc.torque_limit[:ND])
    t = kp * (a * hc.action_scale + dflt - tb.dof_pos.astype(np.float64)) - kd * tb.dof_vel.astype(np.float64)
    return t, lim


def phi_cap(hc):
    """The gap below which the Baumgarte target is cut at vmax: -vmax dt / beta."""
    return -hc.max_depenetration_vel * hc.sim_dt / hc.baumgarte


def branches(tb, hc, model, D, PL):
    base, is_pair = item_slots(model)
    nit = len(base)
    cap = phi_cap(hc)
    caps_kind = [model.capsule_kind[model.pair[p][0]] for p in range(model.num_pairs)]
    box = np.array([bool(is_pair[it]) and caps_kind[it - model.num_leg_contacts] == 1 for it in range(nit)])
    seg = is_pair & ~box
    lim_on, sgn, gap = limit_gaps(tb, model)
    t, lim = pd_torque(tb, hc)
    fixed = bool(hc.fix_base_link)
    out = []
    for e in range(tb.n):
        b = set()
        code, act, kept, phi, nx = D["code"][e], D["active"][e] == 1, PL["kept"][e], D["phi"][e], np.abs(D["normal"][e, :, 0])
        r2 = np.arange(nit) >= 32
        if (act & r2).any():
            b.add("round2_runs")
            if (kept & r2).any() and (kept & ~r2).any():
                b.add("round2_ranks_after_round1")
            mate = e ^ 1
            if mate < tb.n and not (D["active"][mate] == 1)[32:].any():
                b.add("round2_mixed_wave")
        # the plane early-out: no round-2 item of the wave can be active (both envs far above the plane)
        mate = e ^ 1
        far = lambda i: i >= tb.n or (D["phi"][i, 32:nit] > 0.1).all()  # noqa: E731
        if nit > 32 and not fixed and hc.terrain_type == 0 and far(e) and far(mate):
            b.add("round2_skipped")
        if PL["over"][e].any():
            b.add("over_9_points")
        if (lim_on[e] & ~PL["lim_kept"][e]).any():
            b.add("limit_row_dropped")
        order, jf = friction_order(model)
        if any(jf[j] > 0 and not PL["fric_kept"][e, j] for j in range(ND)):
            b.add("friction_row_dropped")
        if PL["lim_kept"][e].any() and PL["fric_kept"][e].any():
            b.add("friction_after_limits")
        for name, m in (("seg_parallel", seg & ((code & P.DS_PARALLEL) != 0)), ("seg_t_below_0", seg & ((code & P.DS_TLO) != 0)),
                        ("seg_t_above_1", seg & ((code & P.DS_THI) != 0)), ("seg_interior", seg & (code == 0)),
                        ("box_inside", box & ((code & P.DS_BOX_INSIDE) != 0))):
            if (m & kept).any():   # counted only where the branch decides a contact that enters the solve
                b.add(name)
        # which end sphere the face is tested against: the thigh's far end (0) reaches the face only
        # with the hip pitched past the horizontal, its near end (1) is the closer one otherwise
        # and never reaches the face, so end 1 is counted wherever it is chosen
        if (box & ((code & P.DS_BOX_END1) == 0) & kept).any():
            b.add("box_end0")
        if (box & ((code & P.DS_BOX_END1) != 0)).any():
            b.add("box_end1")
        if (box & ((code & P.DS_BOX_INSIDE) == 0) & (D["aux"][e, :, 2] < hc.contact_offset)).any():
            b.add("box_outside")   # would be active by its depth: the rectangle test alone rejects it
        if (kept & (nx < 0.9)).any():
            b.add("tangent_ref_x")
        if (kept & (nx >= 0.9)).any():
            b.add("tangent_ref_y")
        if (kept & (phi >= 0)).any():
            b.add("contact_target_speculative")
        if (kept & (phi < 0) & (phi >= cap)).any():
            b.add("contact_target_baumgarte")
        if (kept & (phi < cap)).any():
            b.add("contact_target_vmax")
        lk = PL["lim_kept"][e]
        for name, m in (("limit_lower_approach", (sgn[e] > 0) & (gap[e] >= 0)), ("limit_lower_penetrated", (sgn[e] > 0) & (gap[e] < 0)),
                        ("limit_upper_approach", (sgn[e] < 0) & (gap[e] >= 0)), ("limit_upper_penetrated", (sgn[e] < 0) & (gap[e] < 0)),
                        ("limit_target_vmax", gap[e] < cap)):
            if (lk & m).any():
                b.add(name)
        if (t[e] > lim).any():
            b.add("torque_saturated_pos")
        if (t[e] < -lim).any():
            b.add("torque_saturated_neg")
        if (np.abs(t[e]) <= lim).any():
            b.add("torque_unsaturated")
        if hc.terrain_type == 1 and not fixed:
            g = ~is_pair
            for name, m in (("hf_lower_triangle", (code & P.DC_UPPER) == 0), ("hf_upper_triangle", (code & P.DC_UPPER) != 0),
                            ("hf_clamp_i_low", (code & P.DC_ILO) != 0), ("hf_clamp_i_high", (code & P.DC_IHI) != 0),
                            ("hf_clamp_j_low", (code & P.DC_JLO) != 0), ("hf_clamp_j_high", (code & P.DC_JHI) != 0)):
                sloped = D["normal"][e, :, 2] < 0.9999 if "triangle" in name else True
                if (g & m & kept & sloped).any():
                    b.add(name)
        if not act.any() and tb.root_states[e, 2] > 2 and np.linalg.norm(tb.root_states[e, 10:13]) >= 5:
            b.add("flight_any_orientation")
        out.append(b)
    return out


def margins(tb, hc, model, D, actions=None):
    """kind -> per-row least margin (inf where the row has no decision of that kind)."""
    base, is_pair = item_slots(model)
    nit = len(base)
    cap, off = phi_cap(hc), hc.contact_offset
    caps_kind = [model.capsule_kind[model.pair[p][0]] for p in range(model.num_pairs)]
    box = np.array([bool(is_pair[it]) and caps_kind[it - model.num_leg_contacts] == 1 for it in range(nit)])
    seg = is_pair & ~box
    ground = ~is_pair
    fixed = bool(hc.fix_base_link)
    phi, aux, code, act = D["phi"][:, :nit].astype(np.float64), D["aux"][:, :nit].astype(np.float64), D["code"][:, :nit], D["active"][:, :nit] == 1
    inf = np.inf
    three = lambda x: np.minimum(np.minimum(np.abs(x - off), np.abs(x)), np.abs(x - cap))  # noqa: E731
    live = np.broadcast_to(ground & (not fixed) | seg, phi.shape) | (box[None] & ((code & P.DS_BOX_INSIDE) != 0))
    m = {}
    m["phi"] = np.where(live, three(phi), inf).min(1)
    lim_on, _, gap = limit_gaps(tb, model)
    lo, hi = limits(model)
    q = tb.dof_pos.astype(np.float64)
    # both sides' gaps decide whether a row exists; an existing row's gap also decides its target
    m["limit"] = np.minimum(np.minimum(np.abs(q - lo - LIM_MARGIN), np.abs(hi - q - LIM_MARGIN)),
                            np.where(lim_on, np.minimum(np.abs(gap), np.abs(gap - cap)), inf)).min(1)
    t_raw, s_raw, par = aux[..., 1], aux[..., 2], aux[..., 0]
    st = np.minimum(np.minimum(np.abs(t_raw), np.abs(t_raw - 1)), np.minimum(np.abs(s_raw), np.abs(s_raw - 1)))
    # (a pair more than 5 cm outside the offset places no contact whichever closest points it finds)
    m["seg"] = np.where(seg[None] & (phi < off + 0.05), st, inf).min(1)
    m["par_ok"] = np.where(seg[None] & (phi < off + 0.05), (par < MARGINS["par_lo"]) | (par > MARGINS["par_hi"]), True).all(1)
    # the rectangle decides only where the depth would make the contact active
    m["box"] = np.where(box[None], np.minimum(np.abs(aux[..., 0]), np.where(aux[..., 2] < off + 0.05, np.abs(aux[..., 1]), inf)),
                        inf).min(1)
    m["nx"] = np.where(act, np.abs(np.abs(D["normal"][:, :nit, 0].astype(np.float64)) - 0.9), inf).min(1)
    t, lim = pd_torque(tb, hc, actions)
    m["tau"] = ((np.abs(np.abs(t) - lim) - MARGINS["tau_abs"]) / lim).min(1)
    if hc.terrain_type == 1 and not fixed:
        # inside a clamped border cell u or v sits on the edge by construction: only the diagonal counts
        clamped = (code & (P.DC_ILO | P.DC_IHI | P.DC_JLO | P.DC_JHI | P.DC_UV)) != 0
        fr = np.minimum(np.minimum(aux[..., 1], 1 - aux[..., 1]), np.minimum(aux[..., 2], 1 - aux[..., 2]))
        uv = np.minimum(np.abs(aux[..., 0]), np.where(clamped, inf, fr))
        # a flat cell has one plane on both triangles and beyond its edges: no decision there
        near = phi < off + 0.05
        m["uv"] = np.where(ground[None] & near, uv, inf).min(1)
    else:
        m["uv"] = np.full(tb.n, inf)
    return m


def margin_failures(tb, hc, model, D, actions=None):
    m = margins(tb, hc, model, D, actions)
    fails = []
    for kind, floor in (("phi", MARGINS["phi"]), ("limit", MARGINS["limit"]), ("seg", MARGINS["seg"]), ("box", MARGINS["box"]),
                        ("nx", MARGINS["nx"]), ("tau", MARGINS["tau_rel"]), ("uv", MARGINS["uv"])):
        for e in np.flatnonzero(~(m[kind] >= floor)):
            fails.append(f"row {e} ({tb.names[e]}): {kind} margin {m[kind][e]:.3g} < {floor:g}")
    for e in np.flatnonzero(~m["par_ok"]):
        fails.append(f"row {e} ({tb.names[e]}): denom / (a e) between {MARGINS['par_lo']:g} and {MARGINS['par_hi']:g}")
    return fails


# ---------------------------------------------------------------------------------------- the tables
PAIR_POSES.update({
    # name: (joint angles, the branches the pose is there for)
    "thigh_thigh_t_below_0": ([-0.074, -0.618, -1.216, 0.882, 0.081, -0.012, -0.06, -0.797, 0.998, 0.44, -0.312, -0.216],
                              ("seg_t_below_0", "contact_target_baumgarte")),
    "shin_thigh_t_below_0": ([-0.099, -0.885, 0.338, -0.767, 0.471, -0.141, 0.017, -0.747, -0.398, -0.282, -0.001, -0.129],
                             ("seg_t_below_0",)),
    "thigh_thigh_t_above_1": ([-0.268, -0.49, -0.46, 0.316, -0.597, -0.357, 0.251, 0.059, 1.233, 0.993, -0.575, -0.096],
                              ("seg_t_above_1", "contact_target_vmax")),
    "shin_shin_t_above_1": ([-0.071, 0.083, 0.551, 0.993, 0.773, 0.352, 0.122, 0.053, -0.023, 0.091, -0.672, -0.251],
                            ("seg_t_above_1",)),
    "hand_thigh_t_above_1": ([0.26, 0.5, -0.45, -0.686, 0.638, 0.149, -0.098, 0.119, 0.917, -0.132, 0.012, -0.341],
                             ("seg_t_above_1",)),
    "thigh_thigh_interior": ([-0.165, 0.015, 0.082, 0.978, -0.54, 0.368, 0.248, -0.136, -0.721, 0.118, -0.045, 0.031],
                             ("seg_interior",)),
    "foot_shin_interior": ([-0.097, 0.254, -0.166, -0.855, 0.11, 0.351, 0.06, 0.807, -0.679, -0.712, -0.366, -0.057],
                           ("seg_interior",)),
    "left_hand_thigh": ([0.255, -0.109, 0.996, -0.538, 0.259, 0.242, 0.015, -0.67, 0.223, -1.004, 0.028, -0.307],
                        ("seg_interior",)),
    "right_hand_thigh": ([-0.248, 0.111, -1.155, 0.775, 0.122, 0.03, -0.148, 0.466, 1.389, -0.57, -0.394, -0.059],
                         ("seg_interior",)),
    "box_left_thigh_inside": ([-0.223, 0.694, -1.305, -0.247, -0.059, -0.099, -0.102, -0.242, -1.064, 0.078, -0.017, 0.287],
                              ("box_inside", "box_end0")),
    "box_right_thigh_inside": ([0.006, -0.777, 0.514, -0.207, -0.388, 0.188, -0.076, -0.777, 1.435, -0.998, 0.354, 0.278],
                               ("box_inside", "box_end0", "contact_target_speculative")),
    "box_left_thigh_outside": ([1.186, -0.198, -1.324, 0.483, -0.14, -0.129, 0.213, 0.054, 1.367, 0.981, -0.777, 0.189],
                               ("box_outside",)),
    # both legs rolled the same way until the thigh axes are parallel and the thighs touch; the
    # left roll is past its lower limit (-0.44), the right one inside its range
    "thighs_parallel": ([-1.0919, -0.0164, 0.0035, 0, 0, 0, -1.0228, -0.004, -0.0042, 0, 0, 0], ("seg_parallel",)),
    # the same with the axes 2e-4 rad apart (denom / (a e) = 5e-8) and converging towards the far
    # ends, where a detection without the near-parallel case puts the contact; yawed by 0.6 rad
    # (_pair_rows), which takes its normal away from |n.x| = 0.9
    "thighs_near_parallel": ([-0.95248, 0.13505, 0.16499, 0, 0, 0, -0.96177, -0.00651, -0.1655, 0, 0, 0], ("seg_parallel",)),
    "thighs_parallel_t_below_0": ([0.9547, -0.0198, 0.0012, 0, 0, 0, 1.0235, -0.0081, -0.0021, 0, 0, 0],
                                  ("seg_parallel", "seg_t_below_0")),
})

FALL_V, FALL_W = (0.2, -0.1, -0.3), (0.5, -0.4, 0.3)


def _joint_rows(model, hc):
    """Rows that need no ground: joint limits and torque saturation (in flight on a floating base)."""
    lo, hi = limits(model)
    z = np.zeros(ND)
    rows = []
    # a generic pose: with the base axis-aligned and every joint at exactly 0 most products of the
    # kinematics are exact in fp32, the CPU f32 builds are ten to fifty times more accurate than on
    # the same state turned by a random rotation, and the yardstick they set is one no other fp32
    # order of operations meets (the K_step missed qd of the unsaturated ankle by 46 yardsticks
    # there, at an error that is the MEDIAN of the f32 oracle's own over random rotations)
    off = 0.03 * np.array([1, -2, 3, -1, 2, -3, -2, 1, -3, 2, -1, 3])

    def q_with(**kw):
        q = off.copy()
        for k, v in kw.items():
            q[int(k[1:])] = v
        return q
    rows.append(("limits_all_six", ("limit_lower_approach", "limit_upper_approach", "limit_lower_penetrated",
                                    "limit_upper_penetrated", "limit_target_vmax", "friction_after_limits"),
                 dict(q=q_with(j3=lo[3] + 0.005, j9=hi[9] - 0.005, j4=lo[4] - 0.002, j10=hi[10] + 0.002, j5=lo[5] - 0.008,
                               j11=hi[11] + 0.008))))
    qd = z.copy()
    qd[[1, 7, 3, 9]] = [-2.0, 2.0, 1.5, -1.5]   # into the yaw limits, out of the knee limits
    rows.append(("limits_moving", ("limit_lower_approach", "limit_upper_approach", "limit_lower_penetrated", "limit_upper_penetrated"),
                 dict(q=q_with(j1=lo[1] + 0.004, j7=hi[7] - 0.006, j3=hi[3] + 0.003, j9=lo[9] - 0.004), qd=qd)))
    rows.append(("saturated_by_position", ("torque_saturated_pos", "torque_saturated_neg"), dict(q=q_with(j2=-0.7, j8=0.7))))
    qd = z.copy()
    qd[[4, 10]] = [-10.0, 10.0]
    rows.append(("saturated_by_velocity", ("torque_saturated_pos", "torque_saturated_neg"), dict(q=off, qd=qd)))
    a = z.copy()
    a[[0, 6]] = [2.6, -2.6]   # 130 N m of PD torque against the 85 N m limit
    rows.append(("saturated_by_action", ("torque_saturated_pos", "torque_saturated_neg"), dict(q=off, act=a)))
    rows.append(("almost_saturated", ("torque_unsaturated",), dict(q=q_with(j2=-0.55, j8=0.55, j0=0.38, j6=-0.38))))
    return [(n, t, dict(kw, rpy=(0.4, -0.3, 0.8))) for n, t, kw in rows]


def _pair_rows(yaw=0.0):
    rows = [(name, tg, dict(q=q, rpy=(0, 0, 0.6 if name == "thighs_near_parallel" else yaw))) for name, (q, tg) in PAIR_POSES.items()]
    # the hand-thigh normal is lateral in the base frame: a quarter turn of yaw puts it along world x
    # (the yaw that brings each pose's normal within 0.02 rad of the x axis)
    for name, yw in (("left_hand_thigh", 1.71), ("right_hand_thigh", 1.99), ("hand_thigh_t_above_1", 1.73)):
        rows.append((name + "_yawed", ("tangent_ref_y",), dict(q=PAIR_POSES[name][0], rpy=(0, 0, yw))))
    return rows


def _settle(kw, hc, model, hf, target, body_mass, rank=0):
    """Base height at which the pose's lowest ground candidate (or its rank-th lowest) has the gap
    `target`."""
    kw = dict(kw)
    for _ in range(4):
        t = Table("x")
        t.add("x", (), **kw)
        t.finish(model, 0)
        D = P.detect(hc, model, t.root_states, t.dof_pos, body_mass, heightfield=hf)
        _, is_pair = item_slots(model)
        phi = np.where(is_pair, np.inf, D["phi"][0, :len(is_pair)])
        c = int(np.argsort(phi)[rank])
        kw["z"] = kw["z"] + (target - phi[c]) / max(D["normal"][0, c, 2], 0.5)
    return kw


def _ground_poses(model):
    """(name, branches, pose, target gap of the lowest candidate or None to keep the issue's height)."""
    lo, hi = limits(model)
    rq = np.random.default_rng(7).uniform(-1, 1, (16, ND))
    G = []
    fall = dict(v=FALL_V, w=FALL_W)
    for k, yaw in enumerate((0.0, 0.7, 2.1)):
        G.append((f"face_down_yaw{k}", ("round2_runs", "round2_ranks_after_round1", "round2_mixed_wave", "over_9_points",
),
                  dict(z=0.12, rpy=(0, np.pi / 2, yaw), qd=rq[k], **fall), None))
    for k, yaw in enumerate((0.0, -1.3)):
        G.append((f"squat_yaw{k}", ("over_9_points", "contact_target_vmax"), dict(z=0.1095, rpy=(0, 0, yaw), q=SQUAT, qd=rq[3 + k], **fall), None))
    for k, roll in enumerate((np.pi / 2, -np.pi / 2)):
        G.append((f"on_side{k}", ("over_9_points", "round2_runs"), dict(z=0.12, rpy=(roll, 0, 0.4 * k), qd=rq[5 + k], **fall), None))
    q = np.zeros(ND)
    q[[1, 7, 4, 10, 5, 11]] = [lo[1] - 0.003, hi[7] + 0.003, lo[4] - 0.002, hi[10] + 0.002, lo[5] + 0.004, hi[11] - 0.004]
    G.append(("face_down_six_limits", ("limit_row_dropped", "friction_row_dropped", "over_9_points"),
              dict(z=0.12, rpy=(0, np.pi / 2, 0.3), q=q, **fall), None))
    q = np.zeros(ND)
    q[[1, 7]] = [lo[1] - 0.003, hi[7] + 0.003]
    G.append(("face_down_two_limits", ("friction_after_limits",),
              dict(z=0.12, rpy=(0, np.pi / 2, -0.5), q=q, **fall), None))
    # (the speculative rows approach at 3 and 7 m/s: slower and faster than the 5 m/s that closes
    # their 5 mm gap within the step, and both faster than a Baumgarte target would allow)
    for name, gap, tg, vz in (("standing_speculative", 0.005, "contact_target_speculative", -3.0),
                              ("standing_speculative_fast", 0.005, "contact_target_speculative", -7.0),
                              ("standing_penetrating", -0.002, "contact_target_baumgarte", -0.2),
                              ("standing_deep", -0.008, "contact_target_vmax", -0.2)):
        G.append((name, (tg, "round2_skipped", "tangent_ref_x"), dict(z=0.9, v=(0.3, 0.1, vz), w=(0.1, -0.2, 0.3), qd=rq[8]), gap))
    q = np.zeros(ND)
    q[[1, 7]] = [lo[1] - 0.002, hi[7] + 0.002]
    G.append(("standing_two_limits", ("friction_after_limits",), dict(z=0.9, q=q, qd=rq[9]), -0.001))
    return G


def table(kind, hc, model, hf=None, seed=3):
    """The planted table of `kind` for the config `hc` (decimation does not enter: the margins are
    those of the first substep) and, for "heightfield", the env's own height samples."""
    tb = Table(kind)
    m0 = model.mass[0]
    if kind == "fixed":
        assert hc.fix_base_link
        cases = [(n, t, dict(kw, z=0.95)) for n, t, kw in _pair_rows() + _joint_rows(model, hc)]
        for n, t, kw in cases:
            tb.add(n, t, **kw)
        if len(tb.names) % 2 == 0:
            tb.add("default_pose", ("torque_unsaturated",), z=0.95)
        return tb.finish(model, seed)
    assert not hc.fix_base_link
    if kind == "plane":
        assert hc.terrain_type == 0
        cases = []
        for name, tg, kw, gap in _ground_poses(model):
            cases.append((name, tg, kw if gap is None else _settle(kw, hc, model, None, gap, m0)))
        cases += _pair_rows() + _joint_rows(model, hc)
        return _interleave(tb, cases, seed, hc, model)
    assert kind == "heightfield" and hc.terrain_type == 1 and hf is not None
    rows, cols, hs, border = hc.hf_rows, hc.hf_cols, hc.hf_horizontal_scale, hc.hf_border
    rng = np.random.default_rng(seed)
    H = np.asarray(hf).reshape(rows, cols)
    # cells whose four corners are not coplanar-flat, away from the border, near the origin (small
    # coordinates keep fp32's resolution of (x + border) / scale far below the uv margin)
    i0, i1 = int(border / hs) + 20, int((border + 60) / hs)
    sub = H[i0:i1 + 1, i0:i1 + 1].astype(np.int64)
    sloped = (sub[:-1, :-1] != sub[1:, :-1]) & (sub[:-1, :-1] != sub[:-1, 1:]) & (sub[1:, 1:] != sub[:-1, 1:])
    cells = np.argwhere(sloped) + i0
    assert len(cells) > 100, "no sloped cells in the searched region"
    cases = []
    poses = [g for g in _ground_poses(model) if g[0] in ("face_down_yaw0", "face_down_yaw1", "squat_yaw0", "on_side0", "standing_penetrating",
                                                          "standing_deep", "standing_two_limits")]
    for name, tg, kw, gap in poses * 2:
        want_upper = len(cases) % 2 == 1
        for _ in range(400):
            ci, cj = cells[rng.integers(len(cells))]
            # the base origin somewhere over the chosen cell; the candidates spread from there
            u, v = rng.uniform(0, 1, 2)
            k2 = dict(kw, xy=((ci + u) * hs - border, (cj + v) * hs - border))
            # a fallen pose sinks until its eleventh-lowest candidate is inside the offset (the slope
            # leaves the lower ones centimetres deep: their targets are cut at vmax)
            k2 = _settle(k2, hc, model, hf, 0.004, m0, rank=10) if gap is None else _settle(k2, hc, model, hf, gap, m0)
            t = Table("heightfield")
            t.add(name, tg, **k2)
            t.finish(model, seed)
            D = detect(t, hc, model, hf)
            want = "hf_upper_triangle" if want_upper else "hf_lower_triangle"
            got = branches(t, hc, model, D, plan(t, hc, model, D))[0]
            if not margin_failures(t, hc, model, D) and want in got and (gap is not None or "over_9_points" in got):
                break
        else:
            raise AssertionError(f"no heightfield cell keeps the margins for {name}: {margin_failures(t, hc, model, D)}")
        cases.append((f"{name}_hf{len(cases)}", tuple(x for x in tg if x in got) + (want,), k2))
    # one metre outside the low and the high edge of each axis (index and u / v clamps)
    x_hi, y_hi = (rows - 1) * hs - border, (cols - 1) * hs - border
    mid = 30.03
    stand = [g for g in _ground_poses(model) if g[0] == "standing_penetrating"][0][2]
    for name, xy, tg in (("edge_x_low", (-border - 1.0, mid), "hf_clamp_i_low"), ("edge_x_high", (x_hi + 1.0, mid), "hf_clamp_i_high"),
                         ("edge_y_low", (mid, -border - 1.0), "hf_clamp_j_low"), ("edge_y_high", (mid, y_hi + 1.0), "hf_clamp_j_high")):
        cases.append((name, (tg,), _settle(dict(stand, xy=xy), hc, model, hf, -0.002, m0)))
    return _interleave(tb, cases, seed, hc, model)


# ---------------------------------------------------------------------------------------- verdicts
FIELDS7 = ("q", "qd", "root", "torques", "rigid", "contact", "lam")


class Reference:
    """The f64 step of a table with its fp32 yardstick (oracle/step_tolerance.py), built once and
    shared by every candidate judged on the table."""

    def __init__(self, tb, hc, model, hf=None, a_ref=None, members=3):
        import step_tolerance as ST
        self.ST, self.tb, self.hc, self.model, self.hf = ST, tb, hc, model, hf
        self.a = tb.actions if a_ref is None else a_ref
        self.S = tb.state()
        self.r64 = ST.ref_sim(hc, model, self.S, "f64", hf)
        self.r64.step(self.a)
        self.gap = ST.gap(ST.f32_members(hc, model, self.S, self.a, FIELDS7, hf, members=members), self.r64, FIELDS7)
        self.spread = ST.f64_spread(hc, model, self.S, self.a, self.r64, FIELDS7, hf)
        self.kp, self.kd = np.array(hc.kp[:ND]), np.array(hc.kd[:ND])
        self.D = detect(tb, hc, model, hf)
        self.PL = plan(tb, hc, model, self.D)

    def run(self, precision="f64", library=None):
        """(outputs, dropped) of another build of the oracle on the table."""
        sim = P.RefSim(self.hc, self.model, self.tb.n, precision, heightfield=self.hf, library=library)
        ref = self.ST.ref_sim(self.hc, self.model, self.S, precision, self.hf)
        for k in ("root", "q", "qd", "lam", "mass0", "fric"):
            getattr(sim, k)[:] = getattr(ref, k)
        sim.step(self.a)
        return {f: self.ST.outputs(sim)[f].copy() for f in FIELDS7}, sim.dropped.copy()

    def violations(self, cand, dropped, K=None):
        """Everything the one-substep GPU test asserts, as strings (empty = pass): every element
        inside K x yardstick + rounding (zero outlier envs), finite, the dropped counts equal env
        for env, every slot the detection clears exactly zero.  Returns (violations, headroom)."""
        ST = self.ST
        bad, head, _ = ST.compare(cand, self.r64, self.gap, self.spread, FIELDS7, self.kp, self.kd, ST.STEP_TOL_K if K is None else K)
        out = []
        for e in np.flatnonzero(ST.bad_envs(bad)):
            out.append(f"row {e} ({self.tb.names[e]}) outside the tolerance in {[f for f in FIELDS7 if bad[f][e].any()]}")
        for e in np.flatnonzero(np.asarray(dropped) != self.r64.dropped):
            out.append(f"row {e} ({self.tb.names[e]}) dropped {int(np.asarray(dropped)[e])} rows, the oracle {int(self.r64.dropped[e])}")
        lam = np.asarray(cand["lam"])
        for e in np.flatnonzero(((lam != 0) & self.PL["cleared"]).any(1)):
            out.append(f"row {e} ({self.tb.names[e]}) keeps a warm-start slot the detection clears: "
                       f"{np.flatnonzero((lam[e] != 0) & self.PL['cleared'][e]).tolist()}")
        return out, head


# rows per table (the GPU test sizes its envs by these before it can build a table from them)
SIZES = {"plane": 75, "heightfield": 35, "fixed": 25}
