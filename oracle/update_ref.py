"""numpy references of the update-side kernels (csrc/hg_optim.hip, csrc/hg_mlp.hip, k_gae_norm of
csrc/hg_gae.hip).  TEST INFRASTRUCTURE ONLY: nothing here imports the package.

float64 unless the name ends in 32; the ...32 functions replay IEEE-exact float32 operations in
the kernel's stated order, so the device result is bitwise theirs.

  adam_step64       global-norm clip + Adam over a list of tensors, from the ABI's float32 scalars
  ppo_loss64        the minibatch loss, its parts, the closed-form gradients, the branch distances
  kl_mean64, lr_rule
  elu_bwd32         gy * elu'(y) from the layer output
  tile_partials32   the per-row-tile column sums of k_act_bwd_vec / k_act_bwd_small
  colsum_order32    the three summation orders of the column reductions
  bf16_rne          float32 -> bf16 bit patterns
  skinny_fwd64, skinny_bwd64
  gae_norm32        k_gae_norm from the device's float64 statistics

Every `wrong=` argument selects a deliberately wrong variant; tests/test_update_ref.py shows that
each one moves the result by more than the tolerance the device is held to.

The second half generates the inputs of tests/test_gpu_update_abi.py (adam_case, loss_case, ...),
so that the CPU tests of the references run on exactly what the device runs.
"""
import numpy as np

f32 = np.float32
U24 = 2.0 ** -24
LOG_SQRT_2PI = 0.91893853320467274178
LOG_SQRT_2PI_F32 = f32(LOG_SQRT_2PI)
ADAM_CHUNK = 1024  # hg_adam_chunk()
ACT_RT = 32        # rows per tile of hg_mlp_act_backward
SK_ROWS = 64       # rows per tile of the skinny backward
SK_K = 128


def _w(x):
    """a float32 ABI scalar widened to float64."""
    return float(f32(x))


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
def adam_step64(p, g, m, v, step, lr, b1, b2, eps, max_norm, wrong=None, betas64=None):
    """clip_grad_norm_(params, max_norm); Adam.step() over the list: ONE norm over all tensors,
    coef = min(max_norm / (norm + 1e-6), 1) applied only if max_norm > 0, step + 1, then
      m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
      p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    step: list of floats, or None (the ABI's NULL step pointers: t = 1, nothing incremented).
    Returns a dict of lists p, m, v, step, upd (= p_old - p_new before rounding), m_mag, v_mag
    (the sums of the magnitudes of the two terms of m and v), u_mag (the update with |m| replaced
    by m_mag: what a rounding of m relative to its terms can move), plus coef and norm.
    betas64: (b1, b2) as doubles instead of the widened float32 values (torch's own semantics).
    wrong: "per_tensor_norm", "no_bias_correction", "no_increment"."""
    lr, b1, b2, eps, max_norm = (_w(x) for x in (lr, b1, b2, eps, max_norm))
    if betas64 is not None:
        b1, b2 = betas64
    g64 = [np.asarray(x, np.float64) for x in g]
    norms = [float(np.sqrt((x * x).sum())) for x in g64]
    norm = float(np.sqrt(sum((x * x).sum() for x in g64)))
    out = dict(p=[], m=[], v=[], step=[], upd=[], m_mag=[], v_mag=[], u_mag=[], norm=norm)
    for i, gi in enumerate(g64):
        nrm = norms[i] if wrong == "per_tensor_norm" else norm
        coef = min(max_norm / (nrm + 1e-6), 1.0) if max_norm > 0 else 1.0
        if i == 0:
            out["coef"] = coef
        t = 1.0 if step is None else float(step[i]) + (0.0 if wrong == "no_increment" else 1.0)
        gc = gi * coef
        m0, v0 = np.asarray(m[i], np.float64), np.asarray(v[i], np.float64)
        mi, vi = b1 * m0 + (1 - b1) * gc, b2 * v0 + (1 - b2) * gc * gc
        bc1, bc2 = (np.float64(x) for x in ((1.0, 1.0) if wrong == "no_bias_correction" else (1 - b1 ** t, 1 - b2 ** t)))
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.sqrt(vi) / np.sqrt(bc2) + eps
            upd = lr / bc1 * mi / den
            m_mag = np.abs(b1 * m0) + np.abs((1 - b1) * gc)
            out["u_mag"].append(lr / bc1 * m_mag / den)
        out["p"].append(np.asarray(p[i], np.float64) - upd)
        out["m"].append(mi)
        out["v"].append(vi)
        out["step"].append(t)
        out["upd"].append(upd)
        out["m_mag"].append(m_mag)
        out["v_mag"].append(np.abs(b2 * v0) + (1 - b2) * gc * gc)
    return out


def adam_norm_depth(nblocks):
    """The longest chain of float32 roundings behind the device's squared norm: the square, 3 adds
    in the thread, 6 in the wave, 3 over the block's waves (k_sqnorm); then ceil(nblocks / 256) - 1
    adds in the thread, 6 in the wave and 2 over the waves (k_adam)."""
    return 1 + 3 + 6 + 3 + (-(-nblocks // 256) - 1) + 6 + 2


# ------------------------------------------------------------------------------------------------
# PPO loss
# ------------------------------------------------------------------------------------------------
def _max_w(x, y, wrong):
    tie = 1.0 if wrong == "max_tie_one_side" else 0.5
    return np.where(x > y, 1.0, np.where(x == y, tie, 0.0))


def _max_w2(x, y, wrong):
    """weight of the second argument of max(y, x) (zero on ties in the one-sided wrong variant)."""
    tie = 0.0 if wrong == "max_tie_one_side" else 0.5
    return np.where(x > y, 1.0, np.where(x == y, tie, 0.0))


def _inside(x, lo, hi, wrong):
    return ((x > lo) & (x < hi)) if wrong == "clamp_exclusive" else ((x >= lo) & (x <= hi))


def ppo_loss64(batch, lo, hi, vclip, clipped, c_v, c_e, c_l, wrong=None):
    """The minibatch loss of ppo.py:155-210 and its closed-form gradients, float64 on the float32
    inputs; lo, hi, vclip and the coefficients are the ABI's float32 values widened.
    batch: mu, actions, old_mu, old_sigma [R, A]; std [A]; value, old_logp, advantages,
    target_values, returns [R]; lin_vel, lin_vel_target [R, 3]; optionally ratio_one [R] bool:
    rows whose log-prob difference is exactly zero in the device's float32 by construction (std = 1
    and dyadic a - mu; old_logp is the float32 replay, loss_logp32), which get ratio = 1 here too.
    torch's backward conventions: max gives half to each side on ties, clamp passes on [lo, hi].
    Returns loss, surrogate, value_loss, lin_vel_loss, kl, entropy; g_mu, g_std, g_value, g_lin_vel;
    the error-model quantities ratio, S_lp, d_logp, t_surr, t_v, gs_mag, S_kl; and `dist`, each
    row's relative distance to every branch point (inf where the branch cannot flip: s1 == s2 and
    l1 == l2 are structural inside the band).
    wrong: "max_tie_one_side", "clamp_exclusive", "no_value_clip", "no_entropy_grad", "kl_no_eps"."""
    lo, hi, vclip, c_v, c_e, c_l = (_w(x) for x in (lo, hi, vclip, c_v, c_e, c_l))
    B = {k: np.asarray(x, np.float64) for k, x in batch.items() if k != "ratio_one"}
    mu, s, act = B["mu"], B["std"], B["actions"]
    R, A = mu.shape
    d = act - mu
    q = d * d / (2 * s * s)
    logp = (-q - np.log(s) - LOG_SQRT_2PI).sum(1)
    S_lp = (q + np.abs(np.log(s)) + LOG_SQRT_2PI).sum(1) + np.abs(B["old_logp"])
    ratio = np.exp(logp - B["old_logp"])
    if batch.get("ratio_one") is not None:
        ratio = np.where(batch["ratio_one"], 1.0, ratio)
    adv = B["advantages"]
    rc = np.clip(ratio, lo, hi)
    s1, s2 = -adv * ratio, -adv * rc
    t_surr = np.maximum(s1, s2)
    in_r = _inside(ratio, lo, hi, wrong)
    d_ratio = _max_w(s1, s2, wrong) * -adv + _max_w2(s2, s1, wrong) * -adv * in_r
    d_logp = d_ratio * ratio / R
    g_mu = d_logp[:, None] * d / (s * s)
    gs = d_logp[:, None] * (d * d / s ** 3 - 1 / s)
    gs_mag = np.abs(d_logp)[:, None] * (d * d / s ** 3 + 1 / s)
    g_std = gs.sum(0) - (0.0 if wrong == "no_entropy_grad" else c_e / s)
    # value loss
    v, Rt = B["value"], B["returns"]
    dist = {"ratio_lo": np.abs(ratio - lo) / lo, "ratio_hi": np.abs(ratio - hi) / hi}
    out_r = ~((ratio >= lo) & (ratio <= hi))
    with np.errstate(divide="ignore", invalid="ignore"):
        dist["s1_s2"] = np.where(out_r, np.abs(s1 - s2) / np.maximum(np.abs(s1), np.abs(s2)), np.inf)
    if clipped and wrong != "no_value_clip":
        T = B["target_values"]
        dvt = v - T
        vc = T + np.clip(dvt, -vclip, vclip)
        l1, l2 = (v - Rt) ** 2, (vc - Rt) ** 2
        t_v = np.maximum(l1, l2)
        in_v = _inside(dvt, -vclip, vclip, wrong)
        dv = _max_w(l1, l2, wrong) * 2 * (v - Rt) + _max_w2(l2, l1, wrong) * 2 * (vc - Rt) * in_v
        out_v = np.abs(dvt) > vclip
        dist["v_clip"] = np.abs(np.abs(dvt) - vclip) / vclip
        with np.errstate(divide="ignore", invalid="ignore"):
            dist["l1_l2"] = np.where(out_v, np.abs(l1 - l2) / np.maximum(l1, l2), np.inf)
    else:
        t_v = (Rt - v) ** 2
        dv = 2 * (v - Rt)
    g_v = c_v / R * dv
    e = B["lin_vel"] - B["lin_vel_target"]
    g_p = c_l / (3 * R) * 2 * e
    kl, S_kl = kl_mean64(B["mu"], np.broadcast_to(s, mu.shape), B["old_mu"], B["old_sigma"], wrong=wrong, rows=True)
    ent = float((0.5 + LOG_SQRT_2PI + np.log(s)).sum())
    surr, vl, lv = t_surr.mean(), t_v.mean(), (e * e).sum() / (3 * R)
    return dict(loss=surr + c_v * vl - c_e * ent + c_l * lv, surrogate=surr, value_loss=vl, lin_vel_loss=lv,
                kl=kl.mean(), entropy=ent, g_mu=g_mu, g_std=g_std, g_value=g_v, g_lin_vel=g_p, ratio=ratio,
                S_lp=S_lp, d_logp=d_logp, t_surr=t_surr, t_v=t_v, gs_mag=gs_mag, S_kl=S_kl, dist=dist)


def loss_logp32(act, mu, std):
    """k_ppo_loss_rows' log-prob in float32, action by action.  Bitwise the device's only where no
    transcendental rounds (std == 1: logf(1) = 0) and the compiler has nothing to contract."""
    act, mu, std = (np.asarray(x, f32) for x in (act, mu, std))
    lp = np.zeros(act.shape[0], f32)
    for a in range(act.shape[1]):
        d = act[:, a] - mu[:, a]
        s = std[a]
        lp = lp + ((-(d * d)) / (f32(2) * (s * s)) - np.log(s).astype(f32) - LOG_SQRT_2PI_F32)
    return lp


def kl_mean64(mu, sigma, old_mu, old_sigma, wrong=None, rows=False):
    """mean_rows sum_a [ log(s / s_old + 1e-5) + (s_old^2 + (mu_old - mu)^2) / (2 s^2) - 0.5 ] and the
    mean of the rows' magnitude sums; rows=True returns both per row.  wrong: "kl_no_eps"."""
    mu, s, om, so = (np.asarray(x, np.float64) for x in (mu, sigma, old_mu, old_sigma))
    lg = np.log(s / so + (0.0 if wrong == "kl_no_eps" else _w(1.0e-5)))
    q = (so * so + (om - mu) ** 2) / (2 * s * s)
    kl, S = (lg + q - 0.5).sum(-1), (np.abs(lg) + q + 0.5).sum(-1)
    return (kl, S) if rows else (float(kl.mean()), float(S.mean()))


def lr_rule(kl, lr, desired, lr_min, lr_max):
    """The adaptive-KL rule in float64 on a float32 kl."""
    k = float(f32(kl))
    if k > desired * 2.0:
        return max(lr / 1.5, lr_min)
    if 0.0 < k < desired / 2.0:
        return min(lr * 1.5, lr_max)
    return lr


# ------------------------------------------------------------------------------------------------
# activation backward, column sums, bf16
# ------------------------------------------------------------------------------------------------
def elu_bwd32(gy, y, wrong=None):
    """y > 0 ? gy : gy * (y + 1) in float32 (y the ELU output).  wrong: "elu_y"."""
    gy, y = np.asarray(gy, f32), np.asarray(y, f32)
    fac = y if wrong == "elu_y" else y + f32(1)
    return np.where(y > 0, gy, gy * fac).astype(f32)


def act_lanes(width, vec):
    """row lanes of a 32-row tile: k_act_bwd_vec (256 / min(width / 4, 64)) or k_act_bwd_small."""
    return 256 // min(width // 4, 64) if vec else 256 // width


def tile_partials32(gh, rt, lanes):
    """[ceil(rows / rt), width] float32: per tile, lane rho sums rows rho, rho + lanes, .. of the tile
    in order from 0, then lanes 0, 1, .. are summed in order."""
    gh = np.asarray(gh, f32)
    rows, width = gh.shape
    tiles = -(-rows // rt)
    G = np.zeros((tiles * rt, width), f32)  # + 0 leaves a sum that started at + 0 unchanged
    G[:rows] = gh
    G = G.reshape(tiles, rt, width)
    acc = np.zeros((tiles, lanes, width), f32)
    for i in range(-(-rt // lanes)):
        n = min(lanes, rt - i * lanes)
        acc[:, :n] = acc[:, :n] + G[:, i * lanes:i * lanes + n]
    s = acc[:, 0].copy()
    for k in range(1, lanes):
        s = s + acc[:, k]
    return s


def _tree8(a):
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def colsum_order32(partials, mode, wrong=None):
    """float32 column sums of [parts, width] in the order
      "seq"    p = 0 .. parts - 1;
      "final"  k_colsum_final: 16 lanes, lane l takes parts l, l + 16, ..: rounds of 8 into 8
               accumulators while 8 remain, the rest into accumulator 0, the 8 as a tree, then lanes
               0 .. 15 in order;
      "mod8"   part p into accumulator p % 8 (each in order from 0), the 8 as the same tree.
    wrong: "mod8_shift" (part p into accumulator (p + 1) % 8)."""
    P = np.asarray(partials, f32)
    parts, width = P.shape
    if mode == "seq":
        acc = P[0].copy()
        for p in range(1, parts):
            acc = acc + P[p]
        return acc
    if mode == "mod8":
        s = np.zeros((8, width), f32)
        for p in range(parts):
            k = (p + 1) % 8 if wrong == "mod8_shift" else p % 8
            s[k] = s[k] + P[p]
        return _tree8(s)
    assert mode == "final"
    lanes = []
    for lane in range(16):
        s = np.zeros((8, width), f32)
        t = lane
        while t + 7 * 16 < parts:
            for u in range(8):
                s[u] = s[u] + P[t + 16 * u]
            t += 128
        while t < parts:
            s[0] = s[0] + P[t]
            t += 16
        lanes.append(_tree8(s))
    r = lanes[0]
    for k in range(1, 16):
        r = r + lanes[k]
    return r


def bf16_rne(x, wrong=None):
    """uint16 bf16 bit patterns of float32 x, round-to-nearest-even (inf, signed zeros, subnormals
    exact; NaN stays a NaN).  wrong: "truncate"."""
    b = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    if wrong == "truncate":
        return (b >> 16).astype(np.uint16)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(f32)


# ------------------------------------------------------------------------------------------------
# skinny output layers
# ------------------------------------------------------------------------------------------------
def skinny_fwd64(x, W, b):
    """(y, mag) = x W^T + b and sum_k |x_k W_nk| + |b_n|."""
    x, W, b = (np.asarray(a, np.float64) for a in (x, W, b))
    return x @ W.T + b, np.abs(x) @ np.abs(W).T + np.abs(b)


def _tiles(a, rt):
    """[tiles, rt, ...] zero-padded view of the rows of a."""
    tiles = -(-a.shape[0] // rt)
    out = np.zeros((tiles * rt,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out.reshape((tiles, rt) + a.shape[1:])


def skinny_bwd64(gh, h, W, wrong=None):
    """Per 64-row tile: wb [tiles, n k + n] = [gh^T h, column sums of gh] and wb_mag (the sums of
    the magnitudes); dx = gh W and dx_mag; dx_act = dx * (h > 0 ? 1 : h + 1), and colpart
    [tiles, k] = its column sums per tile with colpart_mag."""
    gh, h, W = (np.asarray(a, np.float64) for a in (gh, h, W))
    n, k = W.shape
    g_t, h_t = _tiles(gh, SK_ROWS), _tiles(h, SK_ROWS)
    dW = np.einsum("trn,trk->tnk", g_t, h_t).reshape(g_t.shape[0], n * k)
    dW_mag = np.einsum("trn,trk->tnk", np.abs(g_t), np.abs(h_t)).reshape(g_t.shape[0], n * k)
    dx, dx_mag = gh @ W, np.abs(gh) @ np.abs(W)
    fac = np.where(h > 0, 1.0, h if wrong == "elu_y" else h + 1.0)
    dx_act = dx * fac
    return dict(wb=np.concatenate([dW, g_t.sum(1)], 1), wb_mag=np.concatenate([dW_mag, np.abs(g_t).sum(1)], 1),
                dx=dx, dx_mag=dx_mag, dx_act=dx_act, fac=fac, colpart=_tiles(dx_act, SK_ROWS).sum(1),
                colpart_mag=_tiles(np.abs(dx_act), SK_ROWS).sum(1),
                colpart_elem=_tiles(dx_mag * np.abs(fac), SK_ROWS).sum(1))


# ------------------------------------------------------------------------------------------------
# GAE normalisation
# ------------------------------------------------------------------------------------------------
def gae_norm32(adv, stats, count):
    """k_gae_norm: mean and unbiased variance in float64 from stats = (sum A, sum A^2) over `count`
    elements (variance clamped at 0), then (A - float(mean)) / (float(std) + 1e-8f) in float32."""
    s0, s1 = float(stats[0]), float(stats[1])
    mean = s0 / count
    var = (s1 - s0 * mean) / (count - 1)
    m = f32(mean)
    d = f32(np.sqrt(var if var > 0.0 else 0.0)) + f32(1e-8)
    return ((np.asarray(adv, f32) - m) / d).astype(f32)


# ================================================================================================
# the bounds the device is held to (u = 2^-24), shared with the discrimination controls
# ================================================================================================
ADAM_C = 14  # roundings behind one element's update, see adam_bounds


def adam_bounds(ref, p_old, step, b1, b2, nblocks):
    """Per tensor, the bounds on |m - m64|, |v - v64| and |(p_new - p_old) - (-upd64)| + rounding of p:
      E    = 0 when the reference does not clip (coef == 1; the cases keep max_norm 1e-4 away from
             the norm); else adam_norm_depth / 2 + 3 (the norm's sum halved by the square root,
             sqrtf, + 1e-6, the division) + 1 (g * coef)
      m    (3 + E) u (|b1 m| + |(1 - b1) g'|)           two products and a sum
      v    (4 + 2 E) u (b2 v + (1 - b2) g'^2)           three products and a sum
      upd  u_mag ((ADAM_C + 2 E) u + u / (2 (1 - b2^t)) + u / (1 - b1^t)) + ulp(p) / 2
           u_mag = the update with |m| replaced by the magnitude sum of m's terms; ADAM_C = 14: m 3,
           sqrt(v) 2 + 1, sqrtf(bc2) 1, the quotient 1, + eps 1, lr / bc1 1, the product and the
           quotient 2, and 2 for the subtractions 1 - b^t below 1/2; the two last terms are powf's
           rounding (1 ulp) in the bias corrections."""
    b1, b2 = _w(b1), _w(b2)
    E = 0.0 if ref["coef"] == 1.0 else adam_norm_depth(nblocks) / 2 + 4
    out = dict(m=[], v=[], upd=[], upd_rel=[], half_ulp=[])  # the two last: upd's two parts, to report
    for i in range(len(ref["p"])):
        t = ref["step"][i]
        out["m"].append((3 + E) * U24 * ref["m_mag"][i])
        out["v"].append((4 + 2 * E) * U24 * ref["v_mag"][i])
        rel = (ADAM_C + 2 * E) * U24 + U24 / (2 * (1 - b2 ** t)) + U24 / (1 - b1 ** t)
        ulp = np.spacing(np.maximum(np.abs(np.asarray(p_old[i], f32)), np.abs(ref["p"][i]).astype(f32)))
        out["upd"].append(ref["u_mag"][i] * rel + 0.5 * ulp.astype(np.float64))
        out["upd_rel"].append(ref["u_mag"][i] * rel)
        out["half_ulp"].append(0.5 * ulp.astype(np.float64))
    return out


def loss_bounds(ref, batch, clipped, c_v, c_e, c_l):
    """Bounds of hg_ppo_loss against ppo_loss64 (R rows, A actions):
      e_lp = (A + 8) u S_lp     log-prob minus old_logp, S_lp the magnitude sum including |old_logp|
      rho  = e_lp + 2^-22        relative error of the ratio (expf within 2 ulp)
      g_mu        |g_mu| (rho + 8 u)      a - mu, s s, 1 / (s s), c_s, four products
      g_value     4 u |g_v| + 2 c_v / R u (|T| + 2 vclip)    (the second: the clipped value's two sums)
      g_lin_vel   4 u |g_p|
      surrogate   mean |t| (rho + 2 u) + u |surrogate|       row terms in float32, summed in float64
      value_loss  4 u mean t_v + mean 2 sqrt(t_v) u (|T| + 2 vclip) + u |value_loss|
      lin_vel     6 u lin_vel_loss
      kl          (A + 8) u mean S_kl + u |kl|
      g_std       sum_r |d_logp| (d^2 / s^3 + 1 / s) (rho + 12 u) + u (|sum| + c_e / s + |g_std|)
      loss        the parts' bounds with their coefficients + u |loss|"""
    c_v, c_e, c_l = (_w(x) for x in (c_v, c_e, c_l))
    R, A = batch["mu"].shape
    u = U24
    rho = (A + 8) * u * ref["S_lp"] + 2.0 ** -22
    vterm = (np.abs(batch["target_values"].astype(np.float64)) + 2 * float(VCLIP)) if clipped else np.zeros(R)
    s = batch["std"].astype(np.float64)
    b = dict(g_mu=np.abs(ref["g_mu"]) * (rho[:, None] + 8 * u),
             g_value=4 * u * np.abs(ref["g_value"]) + 2 * c_v / R * u * vterm,
             g_lin_vel=4 * u * np.abs(ref["g_lin_vel"]),
             surrogate=(np.abs(ref["t_surr"]) * (rho + 2 * u)).mean() + u * abs(ref["surrogate"]),
             value_loss=4 * u * ref["t_v"].mean() + (2 * np.sqrt(ref["t_v"]) * u * vterm).mean() + u * ref["value_loss"],
             lin_vel_loss=6 * u * ref["lin_vel_loss"],
             kl=(A + 8) * u * ref["S_kl"].mean() + u * abs(ref["kl"]))
    col = ref["g_std"] + c_e / s
    b["g_std"] = (ref["gs_mag"] * (rho[:, None] + 12 * u)).sum(0) + u * (np.abs(col) + c_e / s + np.abs(ref["g_std"]))
    b["loss"] = b["surrogate"] + c_v * b["value_loss"] + c_l * b["lin_vel_loss"] + u * abs(ref["loss"])
    return b


def kl_bound(A, S_mean, kl):
    return (A + 8) * U24 * S_mean + U24 * abs(kl)


# ================================================================================================
# inputs of tests/test_gpu_update_abi.py
# ================================================================================================
C_V, C_E, C_L = f32(1.0), f32(0.01), f32(0.5)
# (rows, A, lo, hi, std_one): rows around one wave and past 64 blocks; A up to LOSS_MAX_A; ratio
# exactly on lo and on hi
LOSS_CASES = [(1, 1, 0.8, 1.2, False), (63, 12, 0.8, 1.2, True), (64, 31, 0.8, 1.2, False), (65, 32, 1.0, 1.2, True),
              (65, 12, 0.8, 1.0, True), (4097, 12, 0.8, 1.2, True), (4097, 32, 1.0, 1.2, True), (64, 1, 0.8, 1.0, True)]
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)

# name -> (numels, gradient scale per tensor, starting steps (None: NULL pointers), max_norm as a
# multiple of the float64 norm (None: the literal in the 5th slot), literal max_norm)
ADAM_CASES = {
    "n1": ([1], [1.0], [0.0], None, 0.0),
    "n1023": ([1023], [1.0], [1.0], 0.5, None),
    "n1024": ([1024], [1.0], [999.0], None, -1.0),
    "n1025": ([1025], [1.0], [0.0], 1.0 + 1e-4, None),
    "mixed32": ([1 + (37 * i * i) % 2500 for i in range(32)], [1.0] * 32, [float((0, 1, 999)[i % 3]) for i in range(32)],
                1.0 - 1e-4, None),
    "chunks258": ([257 * 1024 + 1, 5, 1030], [1.0, 1.0, 1.0], [0.0, 1.0, 999.0], 0.25, None),
    "scales": ([700, 1300], [1.0e-4, 1.0], [0.0, 1.0], 0.5, None),
    "zero_grad": ([300, 1025], [0.0, 0.0], [1.0, 1.0], None, 1.0),
    "null_step": ([100, 2049], [1.0, 3.0], None, 0.5, None),
}


def adam_case(name):
    """float32 p, g, m, v lists, step (list or None), lr, b1, b2, eps, max_norm (float32)."""
    numels, scale, step, rel, literal = ADAM_CASES[name]
    rng = np.random.default_rng([11, sorted(ADAM_CASES).index(name)])
    p = [rng.standard_normal(n).astype(f32) for n in numels]
    g = [(sc * rng.standard_normal(n)).astype(f32) for n, sc in zip(numels, scale)]
    ssc = [sc if sc > 0 else 1.0 for sc in scale]  # the moments of a tensor whose gradient is now zero are not
    m = [(0.1 * sc * rng.standard_normal(n)).astype(f32) for n, sc in zip(numels, ssc)]
    v = [(0.01 * sc * sc * rng.random(n)).astype(f32) for n, sc in zip(numels, ssc)]
    norm = float(np.sqrt(sum((x.astype(np.float64) ** 2).sum() for x in g)))
    max_norm = f32(literal) if rel is None else f32(rel * norm)
    return dict(p=p, g=g, m=m, v=v, step=None if step is None else list(step), lr=f32(1e-3), b1=B1, b2=B2, eps=EPS,
                max_norm=max_norm)


def adam_chunks(numels):
    cs = [0]
    for n in numels:
        cs.append(cs[-1] + -(-n // ADAM_CHUNK))
    return cs


PLANTED = ("ratio1", "adv0", "vplus", "vminus", "veq", "ltie")
# which branch distances a planted row is exempt from (it sits ON those branch points, exactly)
PLANTED_EXEMPT = {"ratio1": ("ratio_lo", "ratio_hi", "s1_s2"), "adv0": ("s1_s2",), "vplus": ("v_clip", "l1_l2"),
                  "vminus": ("v_clip", "l1_l2"), "veq": ("l1_l2",), "ltie": ("l1_l2",)}
MARGIN = 1e-4
VCLIP = f32(0.25)  # dyadic: v - T = +-vclip is exact


def loss_case(rows, A, lo=0.8, hi=1.2, std_one=False, seed=0):
    """One minibatch for hg_ppo_loss (all float32, contiguous) with `planted` = {kind: row indices}.
    Ordinary rows: the ratio is spread over [0.55, 1.45] (inside the band and on both sides of it)
    but at least 2e-3 away from 0.8, 1.0 and 1.2; |v - T| in [0.02, 0.6] but not within 2e-3 below
    or 0.02 above vclip; outside the value clip the return is kept 0.1 away from the midpoint of v
    and the clipped value (where l1 == l2); |adv| >= 0.05.  Planted rows (rows >= 16; the ratio ones only
    with std_one, where the log-prob has no transcendental) sit exactly on a branch point:
      ratio1  a - mu = +-0.5, old_logp = the float32 replay: ratio exactly 1 (on lo or hi when they are 1)
      adv0    adv = 0
      vplus / vminus   v - T = +-vclip, dyadic;   veq  v = T
      ltie    v outside the clip and R the midpoint of v and the clipped value: l1 == l2."""
    lo, hi = f32(lo), f32(hi)
    rng = np.random.default_rng([7, rows, A, int(std_one), seed, int(float(lo) * 100), int(float(hi) * 100)])
    std = np.ones(A, f32) if std_one else (0.3 + rng.random(A)).astype(f32)
    mu = rng.standard_normal((rows, A)).astype(f32)
    act = (mu + std * rng.standard_normal((rows, A))).astype(f32)
    d = act.astype(np.float64) - mu
    logp = (-d * d / (2 * std.astype(np.float64) ** 2) - np.log(std.astype(np.float64)) - LOG_SQRT_2PI).sum(1)
    target = 0.55 + 0.9 * rng.random(rows)
    for c in (0.8, 1.0, 1.2):
        near = np.abs(target - c) < 2e-3
        target[near] = c + 4e-3 * np.where(rng.random(near.sum()) < 0.5, -1, 1)
    old_logp = (logp - np.log(target)).astype(f32)
    adv = rng.standard_normal(rows)
    adv = (np.sign(adv) * (0.05 + np.abs(adv))).astype(f32)
    T = rng.standard_normal(rows).astype(f32)
    dvt = 0.02 + 0.58 * rng.random(rows)
    # |l1 - l2| / max(l1, l2) = |v - vc| |v + vc - 2 R| / max >= 0.02 * 0.2 / 3.6^2 = 3e-4 outside the clip
    near = (dvt > float(VCLIP) - 2e-3) & (dvt < float(VCLIP) + 0.02)
    dvt[near] = float(VCLIP) + 0.03
    value = (T + np.where(rng.random(rows) < 0.5, -1, 1) * dvt).astype(f32)
    ret = (T + np.clip(rng.standard_normal(rows), -3, 3)).astype(f32)
    vc = T.astype(np.float64) + np.clip(value.astype(np.float64) - T, -float(VCLIP), float(VCLIP))
    mid = 0.5 * (value.astype(np.float64) + vc)
    close = np.abs(ret - mid) < 0.1
    ret[close] = (mid[close] + 0.3).astype(f32)
    B = dict(mu=mu, std=std, actions=act, old_logp=old_logp, advantages=adv, target_values=T, value=value, returns=ret,
             old_mu=(mu + 0.05 * rng.standard_normal((rows, A))).astype(f32),
             old_sigma=(std * (0.9 + 0.2 * rng.random((rows, A)))).astype(f32),
             lin_vel=rng.standard_normal((rows, 3)).astype(f32), lin_vel_target=rng.standard_normal((rows, 3)).astype(f32))
    planted = {}
    if rows >= 16:
        kinds = [k for k in PLANTED if std_one or k != "ratio1"]
        reps = 2 if rows < 64 else 8
        for i, k in enumerate(kinds):
            planted[k] = np.arange(i * reps, (i + 1) * reps)
        if std_one:
            r = planted["ratio1"]
            sign = np.where((np.arange(A) + r[:, None]) % 2 == 0, 0.5, -0.5).astype(f32)
            act[r] = mu[r] + sign
            # a - mu must come back as +-0.5 exactly: keep mu on a coarse dyadic grid there
            mu[r] = np.round(mu[r] * 8) / 8
            act[r] = mu[r] + sign
            old_logp[r] = loss_logp32(act[r], mu[r], std)
            B["ratio_one"] = np.zeros(rows, bool)
            B["ratio_one"][r] = True
        adv[planted["adv0"]] = 0.0
        for k, dv_, R_ in (("vplus", 0.25, None), ("vminus", -0.25, None), ("veq", 0.0, None), ("ltie", 0.75, 0.5)):
            r = planted[k]
            T[r] = np.round(T[r] * 4) / 4
            value[r] = T[r] + f32(dv_)
            if R_ is not None:
                ret[r] = T[r] + f32(R_)
    return B, planted, float(lo), float(hi)


ACT_Y_EDGES = np.array([0.0, -0.0, -0.5, 0.75, -1.0, -0.999, 1e-30, -1e-30], f32)


def act_case(rows, width, seed=0):
    """(gy, y) float32 [rows, width]; y is an ELU output (> -1) with exact 0.0, -0.0, negative and
    positive values planted along every row."""
    rng = np.random.default_rng([3, rows, width, seed])
    gy = rng.standard_normal((rows, width)).astype(f32)
    h = rng.standard_normal((rows, width))
    y = np.where(h > 0, h, np.expm1(h)).astype(f32)
    flat = y.reshape(-1)
    flat[::5] = np.resize(ACT_Y_EDGES, flat[::5].shape)
    return gy, y


def bf16_round(x):
    """float32 values that are exactly representable in bf16."""
    return bf16_to_f32(bf16_rne(x))


CAST_EDGES = np.array(
    [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,   # ties: to even downwards, upwards, and negative
     0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF,   # just above / below a tie; the largest float32 -> inf
     0x7F800000, 0xFF800000, 0x00000000, 0x80000000,   # inf, signed zeros
     0x00000001, 0x00008000, 0x00018000, 0x807FFFFF,   # subnormals (a tie among them)
     0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFF8000], np.uint32).view(f32)  # NaNs (a carry out of the payload)


def cast_case(count, seed=0):
    rng = np.random.default_rng([5, count, seed])
    x = (rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4, count)).astype(f32)
    x[seed % 3::3] = np.resize(np.roll(CAST_EDGES, seed), x[seed % 3::3].shape)
    return x


def colsum_case(parts, width, seed=0):
    rng = np.random.default_rng([9, parts, width, seed])
    return (rng.standard_normal((parts, width)) * 10.0 ** rng.integers(-2, 3, (parts, 1))).astype(f32)


def skinny_case(rows, n, ldx=SK_K, seed=0):
    """x [rows, ldx] (the first 128 columns are the layer input, an ELU output with planted zeros),
    W [n, 128], b [n], gh [rows, n]."""
    rng = np.random.default_rng([13, rows, n, ldx, seed])
    h = rng.standard_normal((rows, ldx))
    x = np.where(h > 0, h, np.expm1(h)).astype(f32)
    x.reshape(-1)[::7] = np.resize(ACT_Y_EDGES, x.reshape(-1)[::7].shape)
    W = (rng.standard_normal((n, SK_K)) / SK_K ** 0.5).astype(f32)
    return x, W, (0.1 * rng.standard_normal(n)).astype(f32), rng.standard_normal((rows, n)).astype(f32)


# rows around the 256-row block and past 64 blocks (the second pass of k_kl_final); A beyond LOSS_MAX_A
KL_CASES = [(1, 12), (255, 1), (256, 33), (257, 12), (16385, 33), (16385, 1)]


def kl_case(rows, A, seed=0):
    """mu, sigma, old_mu, old_sigma [rows, A] float32; past 64 blocks of 256 rows the means are 8 apart."""
    rng = np.random.default_rng([17, rows, A, seed])
    mu = rng.standard_normal((rows, A)).astype(f32)
    sigma = (0.3 + rng.random((rows, A))).astype(f32)
    old_mu = (mu + 0.1 * rng.standard_normal((rows, A))).astype(f32)
    if rows > 64 * 256:
        # the rows of the blocks past the 64th weigh more than the bound on the mean: a final sum
        # that loses them cannot pass (tests/test_update_ref.py::test_kl_control)
        old_mu[64 * 256:] = mu[64 * 256:] + f32(8)
    return mu, sigma, old_mu, (sigma * (0.8 + 0.4 * rng.random((rows, A)))).astype(f32)


CAST_COUNTS = (1, 3, 4, 1023, 1024, 1025, 4097)

# (parts, width, the order hg_colsum_jobs must use, source offset in floats): 16 jobs, one launch
COLSUM_JOBS = [(1, 5, "seq", 0), (16, 300, "seq", 0), (17, 37, "final", 0), (130, 20, "final", 0),
               (2, 4096, "seq", 0), (16, 4096, "seq", 0), (17, 4096, "mod8", 0), (64, 4096, "mod8", 0),
               (70, 4096, "mod8", 0), (3, 4098, "seq", 0), (17, 4098, "final", 0), (5, 4096, "seq", 1),
               (20, 4096, "final", 1), (131, 16, "final", 0), (1, 4096, "seq", 0), (16, 1, "seq", 0)]
