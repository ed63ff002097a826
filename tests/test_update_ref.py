"""oracle/update_ref.py on the CPU: the references tests/test_gpu_update_abi.py holds the update-side
kernels to, checked against torch float64 (autograd; clip_grad_norm_ + Adam), and shown to
discriminate on the very inputs the device runs.

  closed-form loss gradients   ppo_loss64 against float64 autograd of the ppo.py:155-210 expression,
                               planted ties and boundaries included
  Adam                         adam_step64 against clip_grad_norm_ + torch.optim.Adam(foreach=False)
  discrimination controls      every wrong= variant moves a result by more than the device's bound
  branch margins               every row that is not planted sits > 1e-4 (relative) from every branch
                               point, so the device test leaves out no row or element
"""
import numpy as np
import pytest
import torch

import update_ref as UR

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# the loss
# ------------------------------------------------------------------------------------------------
def _torch_loss(B, lo, hi, vclip, clipped, c_v, c_e, c_l):
    """ppo.py:155-210 written out, float64; returns (loss, parts, gradients)."""
    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in B.items() if k != "ratio_one"}
    mu, std, value, lin_vel = (t[k].clone().requires_grad_(True) for k in ("mu", "std", "value", "lin_vel"))
    dist = torch.distributions.Normal(mu, std.expand_as(mu))
    logp = dist.log_prob(t["actions"]).sum(-1)
    diff = logp - t["old_logp"]
    if B.get("ratio_one") is not None:  # the device's float32 difference is exactly 0 on these rows
        diff = torch.where(torch.tensor(B["ratio_one"]), logp - logp.detach(), diff)
    ratio = torch.exp(diff)
    adv = t["advantages"]
    surrogate = -adv * ratio
    surrogate_clipped = -adv * torch.clamp(ratio, lo, hi)
    surrogate_loss = torch.max(surrogate, surrogate_clipped).mean()
    if clipped:
        T = t["target_values"]
        value_clipped = T + (value - T).clamp(-vclip, vclip)
        value_loss = torch.max((value - t["returns"]).pow(2), (value_clipped - t["returns"]).pow(2)).mean()
    else:
        value_loss = (t["returns"] - value).pow(2).mean()
    entropy = dist.entropy().sum(-1).mean()
    lv = torch.nn.functional.mse_loss(lin_vel, t["lin_vel_target"])
    loss = surrogate_loss + c_v * value_loss - c_e * entropy + c_l * lv
    loss.backward()
    kl = torch.sum(torch.log(std / t["old_sigma"] + float(f32(1e-5)))
                   + (t["old_sigma"].pow(2) + (t["old_mu"] - mu).pow(2)) / (2.0 * std.pow(2)) - 0.5, -1).mean()
    return dict(loss=loss, surrogate=surrogate_loss, value_loss=value_loss, lin_vel_loss=lv, entropy=entropy, kl=kl,
                g_mu=mu.grad, g_std=std.grad, g_value=value.grad, g_lin_vel=lin_vel.grad)


def _loss_args(lo, hi):
    return dict(lo=lo, hi=hi, vclip=UR.VCLIP, c_v=UR.C_V, c_e=UR.C_E, c_l=UR.C_L)


@pytest.mark.parametrize("clipped", [1, 0])
@pytest.mark.parametrize("case", [c for c in UR.LOSS_CASES if c[0] < 4097], ids=str)
def test_loss_gradients_match_autograd(case, clipped):
    B, planted, lo, hi = UR.loss_case(*case)
    ref = UR.ppo_loss64(B, clipped=clipped, **_loss_args(lo, hi))
    tor = _torch_loss(B, lo, hi, float(UR.VCLIP), clipped, float(UR.C_V), float(UR.C_E), float(UR.C_L))
    for k in ("loss", "surrogate", "value_loss", "lin_vel_loss", "entropy", "kl"):
        assert abs(ref[k] - float(tor[k].detach())) <= 1e-12 * max(1.0, abs(ref[k])), k
    for k in ("g_mu", "g_std", "g_value", "g_lin_vel"):
        got, want = ref[k], tor[k].detach().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-15 * max(1.0, np.abs(want).max()), err_msg=k)
    if planted and clipped:  # the planted rows do sit on ties: half gradients exist in the reference
        r = planted["ltie"]
        full = 2 * float(UR.C_V) / case[0] * (B["value"][r].astype(np.float64) - B["returns"][r])
        np.testing.assert_allclose(ref["g_value"][r], 0.5 * full, rtol=1e-14)


def test_planted_rows_are_exact_in_float32():
    """The planted rows' claims in float32: the replayed log-prob equals old_logp bit for bit,
    v - T is exactly +-vclip or 0, l1 == l2 on the tie rows."""
    for case in UR.LOSS_CASES:
        B, planted, lo, hi = UR.loss_case(*case)
        if not planted:
            continue
        if "ratio1" in planted:
            r = planted["ratio1"]
            lp = UR.loss_logp32(B["actions"][r], B["mu"][r], B["std"])
            assert lp.tobytes() == B["old_logp"][r].tobytes()
            assert (np.abs(B["actions"][r] - B["mu"][r]) == 0.5).all() and B["ratio_one"][r].all()
        dvt = B["value"] - B["target_values"]
        assert (dvt[planted["vplus"]] == UR.VCLIP).all() and (dvt[planted["vminus"]] == -UR.VCLIP).all()
        assert (dvt[planted["veq"]] == 0).all() and (B["advantages"][planted["adv0"]] == 0).all()
        r = planted["ltie"]
        vc = B["target_values"][r] + np.clip(dvt[r], -UR.VCLIP, UR.VCLIP)
        assert ((B["value"][r] - B["returns"][r]) ** 2 == (vc - B["returns"][r]) ** 2).all() and (dvt[r] > UR.VCLIP).all()


@pytest.mark.parametrize("case", UR.LOSS_CASES, ids=str)
def test_branch_margins(case):
    """Every row not planted on a branch point is farther than 1e-4 (relative) from each of them;
    a planted row is exempt only from the branch points it sits on.  The ordinary rows are spread
    inside the band and on both sides of it."""
    B, planted, lo, hi = UR.loss_case(*case)
    ref = UR.ppo_loss64(B, clipped=1, **_loss_args(lo, hi))
    rows = case[0]
    for name, dist in ref["dist"].items():
        exempt = np.zeros(rows, bool)
        for kind, r in planted.items():
            if name in UR.PLANTED_EXEMPT[kind]:
                exempt[r] = True
        bad = ~exempt & ~(dist > UR.MARGIN)
        assert not bad.any(), (name, np.nonzero(bad)[0][:8], dist[bad][:8])
    if rows >= 63:
        ratio = ref["ratio"]
        assert (ratio < lo).any() and (ratio > hi).any() and ((ratio > lo) & (ratio < hi)).any()
        dvt = np.abs(B["value"].astype(np.float64) - B["target_values"])
        assert (dvt > UR.VCLIP).any() and (dvt < UR.VCLIP).any()


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.5, 1e6, 0.0, -1.0])
def test_adam_matches_torch(max_norm):
    """Three steps of clip_grad_norm_ + Adam(foreach=False) in float64; two tensors whose gradient
    norms differ by 1e4 (one global norm), fresh gradients every step; max_norm 0.5 clips, 1e6,
    0 and -1 do not (torch is not called to clip for max_norm <= 0: the ABI's rule)."""
    rng = np.random.default_rng(1)
    numels, scales = (700, 1300), (1e-4, 1.0)
    p = [rng.standard_normal(n) for n in numels]
    lr, b1, b2, eps = (float(f32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))
    tp = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in p]
    opt = torch.optim.Adam(tp, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    m, v, step = [np.zeros(n) for n in numels], [np.zeros(n) for n in numels], [0.0, 0.0]
    for it in range(3):
        g = [sc * rng.standard_normal(n) for n, sc in zip(numels, scales)]
        for t, gi in zip(tp, g):
            t.grad = torch.tensor(gi)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(tp, float(f32(max_norm)))
        opt.step()
        ref = UR.adam_step64(p, g, m, v, step, f32(lr), f32(b1), f32(b2), f32(eps), f32(max_norm))
        assert (ref["coef"] < 1.0) == (max_norm == 0.5)
        p, m, v, step = ref["p"], ref["m"], ref["v"], ref["step"]
        assert step == [it + 1.0] * 2
        for i, t in enumerate(tp):
            st = opt.state[t]
            np.testing.assert_allclose(p[i], t.detach().numpy(), rtol=1e-12, atol=1e-16)
            np.testing.assert_allclose(m[i], st["exp_avg"].numpy(), rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(v[i], st["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)
            assert float(st["step"]) == step[i]


# ------------------------------------------------------------------------------------------------
# discrimination controls: on the device test's own inputs, against the device test's own bounds
# ------------------------------------------------------------------------------------------------
def _adam_refs(name, wrong):
    c = UR.adam_case(name)
    a = (c["p"], c["g"], c["m"], c["v"], c["step"], c["lr"], c["b1"], c["b2"], c["eps"], c["max_norm"])
    good, bad = UR.adam_step64(*a), UR.adam_step64(*a, wrong=wrong)
    nblocks = UR.adam_chunks([x.size for x in c["p"]])[-1]
    return good, bad, UR.adam_bounds(good, c["p"], c["step"], c["b1"], c["b2"], nblocks)


@pytest.mark.parametrize("name,wrong,key", [("scales", "per_tensor_norm", "m"), ("scales", "per_tensor_norm", "v"),
                                            ("scales", "per_tensor_norm", "upd"), ("scales", "no_bias_correction", "upd"),
                                            ("chunks258", "no_bias_correction", "upd"), ("n1023", "no_increment", "upd"),
                                            ("mixed32", "no_increment", "upd"), ("chunks258", "no_increment", "upd")])
def test_adam_controls(name, wrong, key):
    good, bad, bound = _adam_refs(name, wrong)
    worst = 0.0
    for g, b, bd in zip(good[key], bad[key], bound[key]):
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(b - g) / bd
        r[~np.isfinite(r)] = np.inf  # t = 0 divides by a zero bias correction: as wrong as it gets
        worst = max(worst, float(r.max()))
    assert worst > 1.0, (name, wrong, key, worst)


def test_adam_cases_keep_the_norm_off_max_norm():
    """Whether a case clips is decided by the reference alone: max_norm is either <= 0, or at least
    1e-4 (relative) away from the norm, 100 times the device norm's worst float32 error."""
    for name in UR.ADAM_CASES:
        c = UR.adam_case(name)
        ref = UR.adam_step64(c["p"], c["g"], c["m"], c["v"], c["step"], c["lr"], c["b1"], c["b2"], c["eps"], c["max_norm"])
        mx = float(c["max_norm"])
        nb = UR.adam_chunks([x.size for x in c["p"]])[-1]
        assert mx <= 0 or abs(mx / (ref["norm"] + 1e-6) - 1.0) > 0.9e-4 > 100 * UR.adam_norm_depth(nb) / 2 * UR.U24
    assert UR.adam_step64(*[UR.adam_case("n1025")[k] for k in ("p", "g", "m", "v", "step", "lr", "b1", "b2", "eps",
                                                                "max_norm")])["coef"] == 1.0
    assert UR.adam_step64(*[UR.adam_case("mixed32")[k] for k in ("p", "g", "m", "v", "step", "lr", "b1", "b2", "eps",
                                                                 "max_norm")])["coef"] < 1.0


@pytest.mark.parametrize("wrong,key,case", [
    ("kl_no_eps", "kl", (64, 31, 0.8, 1.2, False)), ("kl_no_eps", "kl", (1, 1, 0.8, 1.2, False)),
    ("kl_no_eps", "kl", (4097, 32, 1.0, 1.2, True)),
    ("max_tie_one_side", "g_value", (63, 12, 0.8, 1.2, True)), ("clamp_exclusive", "g_value", (64, 31, 0.8, 1.2, False)),
    ("clamp_exclusive", "g_mu", (65, 32, 1.0, 1.2, True)), ("clamp_exclusive", "g_mu", (65, 12, 0.8, 1.0, True)),
    ("clamp_exclusive", "g_std", (65, 12, 0.8, 1.0, True)),
    ("no_value_clip", "g_value", (65, 12, 0.8, 1.0, True)), ("no_value_clip", "value_loss", (4097, 12, 0.8, 1.2, True)),
    ("no_entropy_grad", "g_std", (4097, 32, 1.0, 1.2, True)), ("no_entropy_grad", "g_std", (64, 1, 0.8, 1.0, True)),
    ("no_entropy_grad", "g_std", (64, 31, 0.8, 1.2, False))], ids=str)
def test_loss_controls(wrong, key, case):
    assert case in UR.LOSS_CASES
    B, planted, lo, hi = UR.loss_case(*case)
    good = UR.ppo_loss64(B, clipped=1, **_loss_args(lo, hi))
    bad = UR.ppo_loss64(B, clipped=1, wrong=wrong, **_loss_args(lo, hi))
    bound = UR.loss_bounds(good, B, 1, UR.C_V, UR.C_E, UR.C_L)[key]
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.abs(np.asarray(bad[key]) - good[key]) / bound))
    assert worst > 1.0, (wrong, key, worst)


def test_kl_control():
    """hg_kl_mean's own cases (A = 1, 12, 33): dropping the 1e-5 moves the mean past its bound, and so
    does losing the rows past the 64th block."""
    for rows, A in UR.KL_CASES:
        mu, sg, om, so = UR.kl_case(rows, A)
        kl, S = UR.kl_mean64(mu, sg, om, so)
        bad, _ = UR.kl_mean64(mu, sg, om, so, wrong="kl_no_eps")
        assert abs(bad - kl) > 2 * UR.kl_bound(A, S, kl), (rows, A)
        if rows > 64 * 256:  # a final reduction that stops after 64 blocks
            r, _ = UR.kl_mean64(mu, sg, om, so, rows=True)
            assert r[64 * 256:].sum() / rows > 100 * UR.kl_bound(A, S, kl), (rows, A)


def test_bitwise_controls():
    """The replays the device must match bit for bit: a wrong variant gives other bits on the
    device test's inputs."""
    for rows, width in ((33, 12), (69, 132), (32, 260)):
        gy, y = UR.act_case(rows, width)
        assert UR.elu_bwd32(gy, y).tobytes() != UR.elu_bwd32(gy, y, wrong="elu_y").tobytes()
        assert {0.0, -0.5, 0.75} <= set(y.reshape(-1).tolist()) and np.signbit(y[y == 0]).any()
        assert not np.signbit(y[y == 0]).all() and (y >= -1).all()
    for count in UR.CAST_COUNTS:
        x = UR.cast_case(count, seed=count)
        if count >= 1023:
            assert UR.bf16_rne(x).tobytes() != UR.bf16_rne(x, wrong="truncate").tobytes(), count
    for parts, width, mode, _ in UR.COLSUM_JOBS:
        if mode == "mod8":
            P = UR.colsum_case(parts, width)
            assert UR.colsum_order32(P, "mod8").tobytes() != UR.colsum_order32(P, "mod8", wrong="mod8_shift").tobytes()
    x, W, b, gh = UR.skinny_case(65, 12, 130)
    good, bad = UR.skinny_bwd64(gh, x[:, :128], W), UR.skinny_bwd64(gh, x[:, :128], W, wrong="elu_y")
    assert (np.abs(good["dx_act"] - bad["dx_act"]) > 1e-6 * good["dx_mag"]).any()


# ------------------------------------------------------------------------------------------------
# the float32 replays against plain arithmetic
# ------------------------------------------------------------------------------------------------
def test_bf16_rne_edges():
    x = UR.CAST_EDGES
    got = UR.bf16_rne(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert (got[~nan] == want[~nan]).all()
    assert np.isnan(UR.bf16_to_f32(got[nan])).all() and nan.sum() == 4
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[6] == 0x7F80 and got[7] == 0xFF80  # ties; overflow to inf
    assert got[10] == 0 and got[11] == 0x8000 and got[12] == 0 and got[13] == 0 and got[14] == 2
    rng = np.random.default_rng(0)
    r = rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(f32)
    r = r[~np.isnan(r)]
    want = torch.from_numpy(r.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (UR.bf16_rne(r) == want).all()


@pytest.mark.parametrize("parts", [1, 2, 16, 17, 64, 70, 130, 131])
def test_colsum_orders_are_sums(parts):
    P = UR.colsum_case(parts, 37)
    want, mag = P.astype(np.float64).sum(0), np.abs(P.astype(np.float64)).sum(0)
    for mode in ("seq", "final", "mod8"):
        got = UR.colsum_order32(P, mode)
        assert got.dtype == f32 and (np.abs(got - want) <= max(parts - 1, 0) * UR.U24 * mag).all(), mode
    if parts == 1:
        assert UR.colsum_order32(P, "seq").tobytes() == P[0].tobytes()


@pytest.mark.parametrize("rows,width,vec", [(1, 1, False), (33, 100, False), (69, 256, False), (69, 132, True),
                                            (32, 128, True), (70, 260, True)])
def test_tile_partials_are_sums(rows, width, vec):
    gy, y = UR.act_case(rows, width)
    gh = UR.elu_bwd32(gy, y)
    want = np.where(y > 0, gy.astype(np.float64), gy.astype(np.float64) * (y.astype(np.float64) + 1))
    assert (np.abs(gh - want) <= 2 * UR.U24 * np.abs(want)).all()
    part = UR.tile_partials32(gh, UR.ACT_RT, UR.act_lanes(width, vec))
    assert part.shape == (-(-rows // 32), width)
    for t in range(part.shape[0]):
        blk = gh[32 * t:32 * t + 32].astype(np.float64)
        assert (np.abs(part[t] - blk.sum(0)) <= 31 * UR.U24 * np.abs(blk).sum(0)).all()


def test_gae_norm32():
    rng = np.random.default_rng(4)
    a = rng.standard_normal(1000).astype(f32)
    a64 = a.astype(np.float64)
    got = UR.gae_norm32(a, (a64.sum(), (a64 * a64).sum()), a.size)
    want = (a64 - a64.mean()) / (a64.std(ddof=1) + 1e-8)
    assert np.abs(got - want).max() < 1e-6
    c = np.full(5, f32(1.25))
    assert (UR.gae_norm32(c, (5 * 1.25, 5 * 1.25 ** 2), 5) == 0).all()
    assert UR.lr_rule(0.03, 1e-3, 0.01, 1e-5, 1e-2) == 1e-3 / 1.5 and UR.lr_rule(0.001, 1e-3, 0.01, 1e-5, 1e-2) == 1.5e-3
    assert UR.lr_rule(0.01, 1e-3, 0.01, 1e-5, 1e-2) == 1e-3 and UR.lr_rule(0.0, 1e-3, 0.01, 1e-5, 1e-2) == 1e-3
    assert UR.lr_rule(0.03, 1.2e-5, 0.01, 1e-5, 1e-2) == 1e-5 and UR.lr_rule(0.001, 9e-3, 0.01, 1e-5, 1e-2) == 1e-2
