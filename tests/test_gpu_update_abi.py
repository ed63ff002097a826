"""The update-side kernels (csrc/hg_optim.hip, csrc/hg_mlp.hip, the ABI of csrc/hg_gae.hip) through
their C ABI (humanoid._native), against the numpy references of oracle/update_ref.py, at the
smallest shapes that reach every branch of the kernels.

Two kinds of comparison, neither fitted to the kernels (u = 2^-24):
  bitwise   against a float32 replay of IEEE-exact operations in the order include/hgsim.h states:
            the ELU factor, the per-tile and the three column-sum orders, bf16 round-to-nearest-
            even, the GAE normalisation, the backward's scaling, the planted exact rows of the loss;
  bounded   against float64, by a bound made of u and the operation count, written out in
            update_ref.adam_bounds / loss_bounds / kl_bound and in the tests' docstrings.  The
            inputs (update_ref.*_case) keep every ordinary row > 1e-4 away from every branch point
            (tests/test_update_ref.py asserts it), so no row or element is left out.

What would fail if the kernel were wrong (gap -> test):
  k_act_bwd_small at widths that do not divide 256          -> test_act_backward[3], [12], [100], [127], [130], [255]
  k_act_bwd_vec where width / 4 does not divide 256         -> test_act_backward[132], [160] (gh and the partials bitwise)
  the second column tile of k_act_bwd_vec                   -> test_act_backward[260], [768]
  k_colsum_jobs' narrow path on a wide, misaligned job      -> test_colsum_jobs (4098 columns; 4096 off by one float)
  the 64-part round of k_colsum_jobs' wide == 2 path        -> test_colsum_jobs (64 and 70 parts)
  k_cast_bf16_jobs' scalar path                             -> test_cast_bf16_jobs (odd counts, offset pointers)
  the second pass of k_adam's partial loop                  -> test_adam_step[chunks258]
  the second pass of k_kl_final                             -> test_kl_mean[16385-*]
  the second pass of k_ppo_loss_final's lane loop           -> test_ppo_loss[4097-*]

Every output is allocated with sentinel guards (Flat: elements before and after the payload), which
must be intact afterwards; inputs the ABI strides sit in wider tables whose other columns are
NaN.  Rejections are tested only where the entry point returns HG_ERR_ARG before any launch.

Each item of the gap list was confirmed once against a deliberately altered build (never
committed; every alteration in bounds), which made exactly the named tests fail: one lane fewer
in the small kernel at widths that are no power of two ([12], [100], [127]; at 3, 130 and 255 a
tile gives each lane at most one row, or there is one lane, so that alteration changes nothing
there); the idle lanes' rows added to the sum ([132], [160]); column tiles past the first skipped
([260], [768]); the narrow sequential order reversed on wide jobs (the 4098-column and the offset
4096-column job); the 8-load round reversed (64 and 70 parts); the scalar cast truncating; each
of the three second passes dropped (chunks258; 16385 rows; 4097 rows).

Worst measured ratio of each bound on MI355X (all cases; 1 is the bound):
  Adam          m 0.521, v 0.460, the k_sqnorm partials 0.154; update 0.998, of which p's own half
                ulp is nearly all: what it cannot explain is 0.359 of the bound's relative part.
                Not bounded: the first update is 6.7e-6 of its magnitude off the double-beta form.
  loss          g_mu 0.122, g_std 0.009, g_value 0.546, g_lin_vel 0.562, loss 0.101, surrogate
                0.042, value_loss 0.167, lin_vel_loss 0.247, kl 0.071
  hg_kl_mean    0.022 (identical distributions 0.000)
  grad_bias     0.110 of (rows - 1) u sum |gh|;  hg_colsum_jobs 0.989 of (parts - 1) u sum |partials|
                (two parts without cancellation: one rounding is the whole bound)
  skinny        forward 0.076; dW 0.168, db 0.026, dx 0.225, colpart 0.085; bf16 dx 0.995 (the
                bf16 store's half ulp)
The whole file takes 3.6 s on MI355X (94 tests)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_REPO, "humanoid-gym-with-comments_amd"), os.path.join(_REPO, "oracle"),
           os.path.join(_REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import envlogic_ref as E  # noqa: E402
import update_ref as UR  # noqa: E402
from test_gpu_rollout_abi import DEV, HG_ERR_ARG, IDT, SENT, _bits, _lib, _need_gpu, _same_bits, _stream  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
U24 = UR.U24
REL = 1e-6  # tests/test_gpu_linear.py's stated bound for the float32 linear layers
BF16 = torch.bfloat16
NAN = f32(np.nan)


class Flat:
    """n elements with `off` sentinel elements before and `guard` after (the rollout file's Guarded
    in one dimension, with a movable start for the alignment paths); fill = the initial payload."""

    def __init__(self, n, dtype=torch.float32, off=0, guard=64, fill=None):
        self.n, self.off, self.dtype = int(n), off, dtype
        self.es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((off + self.n + guard,), SENT[self.es], dtype=IDT[self.es], device=DEV)
        if fill is not None:
            self.raw[off:off + self.n] = _bits(np.ascontiguousarray(fill).reshape(-1)).to(DEV)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.off * self.es

    def bits(self):
        host = self.raw.cpu()
        keep = torch.ones_like(host, dtype=torch.bool)
        keep[self.off:self.off + self.n] = False
        assert bool((host[keep] == SENT[self.es]).all()), "a guard element was overwritten"
        return host[self.off:self.off + self.n].contiguous()

    def get(self):
        return self.bits().view(self.dtype)

    def np(self, shape=None):
        a = self.bits().numpy()
        a = a.view({4: np.float32, 2: np.uint16, 1: np.uint8}[self.es])
        return a if shape is None else a.reshape(shape)

    def f64(self):
        return self.bits().numpy().view(np.float64)

    def untouched(self):
        return bool((self.raw == SENT[self.es]).all().item())


def _dev(a, off=0):
    """a device copy of a numpy array, `off` elements into its allocation (pointer, keep-alive)."""
    a = np.ascontiguousarray(a)
    t = torch.zeros(a.size + off, dtype=_bits(a.reshape(-1)[:1]).dtype, device=DEV)
    t[off:] = _bits(a.reshape(-1)).to(DEV)
    return t.data_ptr() + off * a.itemsize, t


def _table(a, ld, col0=0):
    """a [rows, w] as columns [col0, col0 + w) of a [rows, ld] NaN table: (pointer of the slice, keep-alive)."""
    a = np.asarray(a, f32)
    a = a.reshape(a.shape[0], -1)
    t = np.full((a.shape[0], ld), NAN, f32)
    t[:, col0:col0 + a.shape[1]] = a
    p, keep = _dev(t)
    return p + 4 * col0, keep


def _ratio(err, bound):
    """max err / bound, after asserting err <= bound everywhere (bound 0 needs err 0)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ok = err <= bound
    nz = bound > 0
    worst = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    assert ok.all(), f"worst ratio {worst:.3f} ({int((~ok).sum())} of {ok.size} elements over the bound)"
    return worst


def _b16(a):
    """uint16 bit patterns as the int16 array torch can take."""
    return np.ascontiguousarray(a, np.uint16).view(np.int16)


# ------------------------------------------------------------------------------------------------
# hg_adam_step
# ------------------------------------------------------------------------------------------------
def _adam_fn():
    from humanoid.algo.ppo.hg_adam import _TensorList
    L = _lib()
    L.hg_adam_step.restype = ctypes.c_int
    L.hg_adam_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                               ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    assert L.hg_adam_chunk() == UR.ADAM_CHUNK
    return L.hg_adam_step, _TensorList


class AdamState:
    def __init__(self, c):
        self.c = c
        self.numels = [x.size for x in c["p"]]
        self.cs = UR.adam_chunks(self.numels)
        self.P, self.M, self.V = ([Flat(x.size, fill=x, guard=32) for x in c[k]] for k in ("p", "m", "v"))
        self.G = [_dev(x) for x in c["g"]]
        self.S = None if c["step"] is None else [Flat(1, fill=np.array([s], f32), guard=4) for s in c["step"]]
        self.lr = _dev(np.array([c["lr"]], f32))
        self.partial = Flat(self.cs[-1], guard=32)
        _, TL = _adam_fn()
        T = TL()
        T.count = len(self.numels)
        for i, n in enumerate(self.numels):
            T.param[i], T.grad[i], T.exp_avg[i], T.exp_avg_sq[i] = self.P[i].ptr, self.G[i][0], self.M[i].ptr, self.V[i].ptr
            T.step[i] = None if self.S is None else self.S[i].ptr
            T.numel[i] = n
        for i, s in enumerate(self.cs):
            T.chunk_start[i] = s
        self.T = T

    def call(self, T=None, lr=True, partial=True, max_norm=None):
        fn, _ = _adam_fn()
        c = self.c
        return fn(ctypes.byref(T or self.T), self.lr[0] if lr else None, float(c["b1"]), float(c["b2"]), float(c["eps"]),
                  float(c["max_norm"] if max_norm is None else max_norm), self.partial.ptr if partial else None, _stream())

    def read(self):
        return ([x.np() for x in self.P], [x.np() for x in self.M], [x.np() for x in self.V],
                None if self.S is None else [float(s.np()[0]) for s in self.S])


@pytest.mark.parametrize("name", sorted(UR.ADAM_CASES))
def test_adam_step(name):
    """Three consecutive hg_adam_step calls, each compared with adam_step64 from the device's own
    state before it (errors do not compound), within update_ref.adam_bounds:
      m    (3 + E) u (|b1 m| + |(1 - b1) g'|);   v   (4 + 2 E) u (b2 v + (1 - b2) g'^2)
      p_new - p_old   u_mag ((14 + 2 E) u + u / (2 (1 - b2^t)) + u / (1 - b1^t)) + ulp(p) / 2
    with E = 0 unless the reference clips (then the norm's summation depth / 2 + 4), u_mag the
    update with |m| replaced by the magnitude sum of its terms.  The k_sqnorm partials left in
    `partial` against the float64 sum of squares of their chunk within 13 u.  Step counters rise
    by exactly 1.0 (a NULL step pointer: t = 1); gradients and lr bitwise unchanged; p, m, v
    beyond numel and partial beyond the chunk count keep their sentinels.
    Cases: 1 / 1023 / 1024 / 1025 elements; 32 tensors; 258 chunks (the second pass of k_adam's
    partial loop); gradient norms 1e4 apart under one global clip; zero gradients; max_norm 0 and
    negative (no clipping), 1e-4 above and below the norm; steps from 0, 1, 999, per tensor.
    Not bounded, only printed: the deviation from torch's semantics, where the bias corrections
    come from the double betas (1 - 0.999f is 1.3e-5 off 1e-3: about 6e-6 of the step-1 update).
    Measured ratios: the head of this file."""
    _need_gpu()
    c = UR.adam_case(name)
    st = AdamState(c)
    nb = st.cs[-1]
    worst = dict(m=0.0, v=0.0, upd=0.0, upd_rel=0.0, partial=0.0)
    dev_torch = 0.0
    for it in range(3):
        p0, m0, v0, s0 = st.read()
        ref = UR.adam_step64(p0, c["g"], m0, v0, s0, c["lr"], c["b1"], c["b2"], c["eps"], c["max_norm"])
        bound = UR.adam_bounds(ref, p0, s0, c["b1"], c["b2"], nb)
        assert st.call() == 0
        torch.cuda.synchronize()
        p1, m1, v1, s1 = st.read()
        if s0 is not None:
            assert s1 == [s + 1.0 for s in s0] == ref["step"]
        for i in range(len(p0)):
            worst["m"] = max(worst["m"], _ratio(np.abs(m1[i] - ref["m"][i]), bound["m"][i]))
            worst["v"] = max(worst["v"], _ratio(np.abs(v1[i] - ref["v"][i]), bound["v"][i]))
            d = p1[i].astype(np.float64) - p0[i].astype(np.float64)
            worst["upd"] = max(worst["upd"], _ratio(np.abs(d + ref["upd"][i]), bound["upd"][i]))
            nz = bound["upd_rel"][i] > 0  # reported only: the part of the error that p's own rounding cannot explain
            if nz.any():
                over = np.clip(np.abs(d + ref["upd"][i]) - bound["half_ulp"][i], 0, None)
                worst["upd_rel"] = max(worst["upd_rel"], float((over[nz] / bound["upd_rel"][i][nz]).max()))
            assert _same_bits(st.G[i][1].cpu(), c["g"][i])
        assert _same_bits(st.lr[1].cpu(), np.array([c["lr"]], f32))
        part = st.partial.np()
        for i, g in enumerate(c["g"]):
            sq = np.zeros((st.cs[i + 1] - st.cs[i]) * UR.ADAM_CHUNK)
            sq[:g.size] = g.astype(np.float64) ** 2
            want = sq.reshape(-1, UR.ADAM_CHUNK).sum(1)
            worst["partial"] = max(worst["partial"], _ratio(np.abs(part[st.cs[i]:st.cs[i + 1]] - want), 13 * U24 * want))
        if it == 0 and s0 is not None:
            tor = UR.adam_step64(p0, c["g"], m0, v0, s0, c["lr"], c["b1"], c["b2"], c["eps"], c["max_norm"],
                                 betas64=(0.9, 0.999))
            for a, b, mag in zip(ref["upd"], tor["upd"], ref["u_mag"]):
                nz = mag > 0
                if nz.any():
                    dev_torch = max(dev_torch, float(np.max(np.abs(a - b)[nz] / mag[nz])))
    print(f"adam {name}: worst ratio m {worst['m']:.3f}, v {worst['v']:.3f}, update {worst['upd']:.3f} "
          f"(beyond p's half ulp: {worst['upd_rel']:.3f} of the relative part), "
          f"partial {worst['partial']:.3f}; first update off the double-beta form by {dev_torch:.2e} of its magnitude (not bounded)")


def test_adam_rejections():
    """count 0 and 33, a NULL lr / partial / tensor pointer, a chunk_start that does not match numel:
    HG_ERR_ARG before any launch, every buffer as it was."""
    _need_gpu()
    _, TL = _adam_fn()
    c = UR.adam_case("null_step")
    st = AdamState(c)

    def variant(f):
        T = TL.from_buffer_copy(st.T)
        f(T)
        return T

    def setf(field, i, val):
        return lambda T: getattr(T, field).__setitem__(i, val)

    bad = [dict(T=variant(lambda T: setattr(T, "count", 0))), dict(T=variant(lambda T: setattr(T, "count", 33))),
           dict(lr=False), dict(partial=False)]
    bad += [dict(T=variant(setf(f, 1, None))) for f in ("param", "grad", "exp_avg", "exp_avg_sq")]
    bad += [dict(T=variant(setf("chunk_start", 2, st.cs[2] + 1))), dict(T=variant(setf("chunk_start", 1, 2))),
            dict(T=variant(setf("numel", 0, 1025)))]
    for kw in bad:
        assert st.call(**kw) == HG_ERR_ARG, kw
    torch.cuda.synchronize()
    assert st.partial.untouched()
    p, m, v, _ = st.read()
    for k, got in (("p", p), ("m", m), ("v", v)):
        for a, b in zip(got, c[k]):
            assert _same_bits(a, b)
    assert st.call() == 0  # the unmodified arguments are valid
    torch.cuda.synchronize()
    st.read()


# ------------------------------------------------------------------------------------------------
# hg_ppo_loss / _lr / _backward
# ------------------------------------------------------------------------------------------------
ROWWISE = ("mu", "value", "lin_vel", "lin_vel_target", "actions", "old_logp", "advantages", "target_values", "returns",
           "old_mu", "old_sigma")


class LossCase:
    def __init__(self, case, strided=False):
        from humanoid.algo.ppo.hg_loss import _Batch
        self.B, self.planted, self.lo, self.hi = UR.loss_case(*case)
        self.rows, self.A = case[0], case[1]
        self.keep = []
        b = _Batch()
        for i, k in enumerate(ROWWISE):
            a = self.B[k].reshape(self.rows, -1)
            w = a.shape[1]
            ld, c0 = (w + 1 + i, i % 3 if i else 0) if strided else (w, 0)  # c0 + w <= ld
            p, keep = _table(a, ld, c0)
            self.keep.append(keep)
            setattr(b, k, p)
            setattr(b, k + "_ld", ld)
        p, keep = _dev(self.B["std"])
        self.keep.append(keep)
        b.std = p
        self.b = b
        self.nscratch = int(_lib().hg_ppo_loss_scratch(self.rows, self.A))
        assert self.nscratch == -(-self.rows // 64) * (4 + self.A)

    def outputs(self, stats=None):
        r, A = self.rows, self.A
        return dict(loss=Flat(1, guard=4), stats=Flat(4, guard=4, fill=stats), g_mu=Flat(r * A), g_std=Flat(A, guard=8),
                    g_value=Flat(r), g_lin_vel=Flat(r * 3), scratch=Flat(2 * self.nscratch))

    def call(self, o, clipped=1, accumulate=0, lr=None, batch=None, rows=None, A=None, null=()):
        L = _lib()
        p = {k: (None if k in null else v.ptr) for k, v in o.items()}
        head = (ctypes.byref(batch or self.b), self.rows if rows is None else rows, self.A if A is None else A,
                self.lo, self.hi, float(UR.VCLIP), clipped, float(UR.C_V), float(UR.C_E), float(UR.C_L), p["loss"],
                p["stats"], accumulate, p["g_mu"], p["g_std"], p["g_value"], p["g_lin_vel"], p["scratch"])
        if lr is None:
            return L.hg_ppo_loss(*head, _stream())
        lr64, lr32, desired, lr_min, lr_max = lr
        return L.hg_ppo_loss_lr(*head, lr64, lr32, desired, lr_min, lr_max, _stream())

    def run(self, **kw):
        o = self.outputs(kw.pop("stats", None))
        assert self.call(o, **kw) == 0
        torch.cuda.synchronize()
        o["scratch"].bits()  # its guards
        return {k: v.np() for k, v in o.items() if k != "scratch"}


def _check_loss(lc, got, clipped):
    """every output of one launch against ppo_loss64 within loss_bounds; returns the ratios."""
    ref = UR.ppo_loss64(lc.B, lc.lo, lc.hi, UR.VCLIP, clipped, UR.C_V, UR.C_E, UR.C_L)
    bound = UR.loss_bounds(ref, lc.B, clipped, UR.C_V, UR.C_E, UR.C_L)
    r, A = lc.rows, lc.A
    out = {}
    for k, shape in (("g_mu", (r, A)), ("g_std", (A,)), ("g_value", (r,)), ("g_lin_vel", (r, 3))):
        out[k] = _ratio(np.abs(got[k].reshape(shape) - ref[k]), bound[k])
    out["loss"] = _ratio(abs(got["loss"][0] - ref["loss"]), bound["loss"])
    for i, k in enumerate(("value_loss", "surrogate", "lin_vel_loss", "kl")):
        out[k] = _ratio(abs(got["stats"][i] - ref[k]), bound[k])
    return out


def _check_planted(lc, got, clipped):
    """the planted rows against a float32 replay, bitwise (every operation on them is exact or a
    single rounding): g_value on v - T = +-vclip, v = T and the l1 == l2 tie; g_mu on ratio == 1."""
    B, pl, rows = lc.B, lc.planted, lc.rows
    if not pl:
        return
    a = (B["value"] - B["returns"]).astype(f32)
    if clipped:
        c_v = f32(float(UR.C_V) / rows)
        for k, fac in (("vplus", 2), ("vminus", 2), ("veq", 2), ("ltie", 1)):
            r = pl[k]
            assert _same_bits(got["g_value"][r], (c_v * (f32(fac) * a[r])).astype(f32)), k
    if "ratio1" in pl:
        r = pl["ratio1"]
        d_logp = (f32(1.0 / rows) * -B["advantages"][r]).astype(f32)
        want = (d_logp[:, None] * (B["actions"][r] - B["mu"][r])).astype(f32)
        assert _same_bits(got["g_mu"].reshape(rows, lc.A)[r], want), "ratio exactly 1 (on lo / hi when they are 1)"


@pytest.mark.parametrize("case", UR.LOSS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_ppo_loss(case):
    """hg_ppo_loss against ppo_loss64 within update_ref.loss_bounds (formulas there: the log-prob
    budget (A + 8) u S, the ratio that plus 2 ulp of expf, g_mu that plus 8 u, g_value / g_lin_vel
    4 u, the float64 sums of float32 row terms their row-term error times the magnitude sum plus
    u for the float store), every row and element, for both clipped_value_loss values; the planted
    exact rows bitwise against their float32 replay; the same data as column slices of wider NaN
    tables with a different stride and offset each: every output bitwise the contiguous launch's;
    accumulate_stats = 1 on prefilled stats adds the three losses in float32 and SETS stats[3].
    rows 4097 is 65 blocks: the second pass of k_ppo_loss_final's lane loop.  A = 32 = LOSS_MAX_A.
    Measured ratios: the head of this file."""
    _need_gpu()
    lc = LossCase(case)
    ls = LossCase(case, strided=True)
    for clipped in (1, 0):
        got = lc.run(clipped=clipped)
        ratios = _check_loss(lc, got, clipped)
        _check_planted(lc, got, clipped)
        got_s = ls.run(clipped=clipped)
        for k in got:
            assert _same_bits(got[k], got_s[k]), ("strided", k)
        pre = np.array([0.5, -1.25, 3.0, 7.0], f32)
        acc = lc.run(clipped=clipped, accumulate=1, stats=pre)
        assert _same_bits(acc["stats"][:3], (pre[:3] + got["stats"][:3]).astype(f32))
        assert _same_bits(acc["stats"][3:], got["stats"][3:])
        for k in got:
            if k != "stats":
                assert _same_bits(got[k], acc[k]), ("accumulate", k)
        print(f"loss {case} clipped={clipped}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_ppo_loss_lr():
    """hg_ppo_loss_lr: every output bitwise hg_ppo_loss's, and (lr64, lr32) bitwise hg_kl_lr_rule on
    stats[3] (and update_ref.lr_rule): KL above, inside and below the band, lr at its floor and cap."""
    _need_gpu()
    L = _lib()
    lc = LossCase(UR.LOSS_CASES[3])
    base = lc.run()
    kl = float(base["stats"][3])
    assert kl > 0
    for desired, lr0, lr_min, lr_max in ((kl / 4, 1e-3, 1e-5, 1e-2), (kl, 1e-3, 1e-5, 1e-2), (kl * 4, 1e-3, 1e-5, 1e-2),
                                         (kl / 4, 1.2e-5, 1e-5, 1e-2), (kl * 4, 9e-3, 1e-5, 1e-2)):
        a64, a32 = Flat(2, guard=4, fill=np.array([lr0], np.float64).view(f32)), Flat(1, guard=4)
        o = lc.outputs()
        assert lc.call(o, lr=(a64.ptr, a32.ptr, desired, lr_min, lr_max)) == 0
        b64, b32 = Flat(2, guard=4, fill=np.array([lr0], np.float64).view(f32)), Flat(1, guard=4)
        klp, keep = _dev(base["stats"][3:])
        assert L.hg_kl_lr_rule(klp, b64.ptr, b32.ptr, desired, lr_min, lr_max, _stream()) == 0
        torch.cuda.synchronize()
        for k in base:
            assert _same_bits(o[k].np(), base[k]), k
        want = UR.lr_rule(base["stats"][3], lr0, desired, lr_min, lr_max)
        assert a64.f64()[0] == b64.f64()[0] == want and _same_bits(a32.np(), b32.np())
        assert a32.np()[0] == f32(want)
    # rejected without the lr pointers, outputs untouched
    o = lc.outputs()
    a64 = Flat(2, guard=4)
    assert lc.call(o, lr=(None, a64.ptr, 0.01, 1e-5, 1e-2)) == HG_ERR_ARG
    assert lc.call(o, lr=(a64.ptr, None, 0.01, 1e-5, 1e-2)) == HG_ERR_ARG
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values()) and a64.untouched()


@pytest.mark.parametrize("rows,A", [(5, 3), (8192, 32)])
def test_ppo_loss_backward(rows, A):
    """Every element of the four gradients is exactly float32(g * s) for a scalar that is not 1;
    8192 x 32 is more than 1024 x 256 elements: the grid stride wraps."""
    _need_gpu()
    rng = np.random.default_rng([rows, A])
    g = {k: rng.standard_normal(n).astype(f32) for k, n in (("mu", rows * A), ("std", A), ("v", rows), ("p", rows * 3))}
    o = {k: Flat(v.size, fill=v) for k, v in g.items()}
    s = np.array([0.37], f32)
    sp, keep = _dev(s)
    assert _lib().hg_ppo_loss_backward(sp, rows, A, o["mu"].ptr, o["std"].ptr, o["v"].ptr, o["p"].ptr, _stream()) == 0
    torch.cuda.synchronize()
    for k in g:
        assert _same_bits(o[k].np(), (g[k] * s[0]).astype(f32)), k
    o2 = {k: Flat(v.size, fill=v) for k, v in g.items()}
    for bad in ("s", "mu", "std", "v", "p", "rows", "A"):
        a = [None if bad == "s" else sp, 0 if bad == "rows" else rows, 0 if bad == "A" else A] + \
            [None if bad == k else o2[k].ptr for k in ("mu", "std", "v", "p")]
        assert _lib().hg_ppo_loss_backward(*a, _stream()) == HG_ERR_ARG, bad
    torch.cuda.synchronize()
    for k in g:
        assert _same_bits(o2[k].np(), g[k]), k


def test_ppo_loss_rejections():
    """Each NULL pointer the code lists, rows = 0, A = 0, A = 33; NULL target_values only when the
    value loss is clipped.  Outputs untouched."""
    _need_gpu()
    from humanoid.algo.ppo.hg_loss import _Batch
    lc = LossCase(UR.LOSS_CASES[1])
    o = lc.outputs()
    for k in o:
        assert lc.call(o, null=(k,)) == HG_ERR_ARG, k
    for kw in (dict(rows=0), dict(A=0), dict(A=33)):
        assert lc.call(o, **kw) == HG_ERR_ARG, kw
    for k in ROWWISE + ("std",):
        b = _Batch.from_buffer_copy(lc.b)
        setattr(b, k, None)
        assert lc.call(o, batch=b, clipped=1) == HG_ERR_ARG, k
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values())
    b = _Batch.from_buffer_copy(lc.b)
    b.target_values = None
    want = lc.run(clipped=0)
    o = lc.outputs()
    assert lc.call(o, batch=b, clipped=0) == 0
    torch.cuda.synchronize()
    for k in want:
        assert _same_bits(o[k].np(), want[k]), k


# ------------------------------------------------------------------------------------------------
# hg_kl_mean
# ------------------------------------------------------------------------------------------------
def _kl(arrs, rows, A, null=None):
    ptrs = [_dev(a) for a in arrs]
    out, scratch = Flat(1, guard=4), Flat(2 * -(-rows // 256), guard=8)
    a = [p for p, _ in ptrs] + [rows, A, out.ptr, scratch.ptr]
    if null is not None:
        a[null] = None if null not in (4, 5) else 0
    rc = _lib().hg_kl_mean(*a, _stream())
    torch.cuda.synchronize()
    return rc, out, scratch


@pytest.mark.parametrize("rows,A", UR.KL_CASES)
def test_kl_mean(rows, A):
    """hg_kl_mean against kl_mean64 within (A + 8) u mean(S) + u |kl| (S the row's magnitude sum:
    the float32 row sums of A terms of a few roundings each; the float64 block and final sums add
    nothing; u for the float store); scratch guarded at ceil(rows / 256) doubles.  16385 rows is 65
    blocks: the second pass of k_kl_final.  Identical old and new distributions give A log(1 +
    1e-5f) within the same bound.  Measured ratios: the head of this file."""
    _need_gpu()
    arrs = UR.kl_case(rows, A)
    rc, out, scratch = _kl(arrs, rows, A)
    assert rc == 0
    kl, S = UR.kl_mean64(*arrs)
    r1 = _ratio(abs(out.np()[0] - kl), UR.kl_bound(A, S, kl))
    scratch.bits()
    rc, out, _ = _kl((arrs[0], arrs[1], arrs[0], arrs[1]), rows, A)
    want = A * np.log(float(f32(1) + f32(1e-5)))
    r2 = _ratio(abs(out.np()[0] - want), UR.kl_bound(A, A * (want / A + 1.0), want))
    assert rc == 0 and out.np()[0] > 0
    print(f"kl rows={rows} A={A}: worst ratio {r1:.3f}; identical distributions {r2:.3f}")
    if rows == 257:
        for null in range(8):
            rc, out, scratch = _kl(arrs, rows, A, null=null)
            assert rc == HG_ERR_ARG and out.untouched() and scratch.untouched(), null


# ------------------------------------------------------------------------------------------------
# hg_mlp_act_backward / _bf16
# ------------------------------------------------------------------------------------------------
def _act_call(bf, gy, y, rows, width, with_gb=True, off=0, null_gh=False):
    """one launch; returns (rc, gh, grad_bias, scratch) as Flat buffers."""
    L = _lib()
    fn = L.hg_mlp_act_backward_bf16 if bf else L.hg_mlp_act_backward
    dt = BF16 if bf else torch.float32
    up = (lambda a: _dev(_b16(UR.bf16_rne(a)), off)) if bf else (lambda a: _dev(a, off))
    gyp = up(gy)
    yp = up(y) if y is not None else (None, None)
    gh = Flat(rows * width, dt, off=off)
    gb = Flat(width, guard=16)
    scratch = Flat(int(L.hg_mlp_act_backward_scratch(max(rows, 1), width)), guard=64)
    rc = fn(gyp[0], yp[0], None if (y is None or null_gh) else gh.ptr, rows, width, gb.ptr if with_gb else None,
            scratch.ptr, _stream())
    torch.cuda.synchronize()
    return rc, gh, gb, scratch


def _act_check(bf, rows, width, vec, off=0):
    gy, y = UR.act_case(rows, width)
    if bf:
        gy, y = UR.bf16_round(gy), UR.bf16_round(y)
    tiles = -(-rows // UR.ACT_RT)
    gh32 = UR.elu_bwd32(gy, y)
    lanes = UR.act_lanes(width, vec)
    worst = 0.0
    for with_y, with_gb in ((True, True), (True, False), (False, True)):
        rc, gh, gb, scratch = _act_call(bf, gy, y if with_y else None, rows, width, with_gb, off)
        assert rc == 0
        src = gh32 if with_y else gy
        if with_y:
            want = _b16(UR.bf16_rne(gh32)) if bf else gh32
            assert _same_bits(gh.bits().numpy().reshape(rows, width), want), "gh"
        else:
            assert gh.untouched()
        part = scratch.np((tiles, width))
        assert _same_bits(part, UR.tile_partials32(src, UR.ACT_RT, lanes)), "per-tile partials"
        if with_gb:
            got = gb.np()
            assert _same_bits(got, UR.colsum_order32(part, "final")), "grad_bias"
            s64 = src.astype(np.float64)
            worst = max(worst, _ratio(np.abs(got - s64.sum(0)), max(rows - 1, 0) * U24 * np.abs(s64).sum(0)))
        else:
            assert gb.untouched()
    return worst


SMALL_W = [1, 3, 12, 100, 127, 130, 255, 256]
VEC_W = [128, 132, 160, 256, 260, 768]


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("width", SMALL_W + VEC_W)
def test_act_backward(width, bf):
    """gh bitwise elu_bwd32 (bf16: bitwise bf16_rne of the float32 product), the per-tile partials
    in scratch bitwise tile_partials32 (lane rho sums rows rho, rho + L, .. of the 32-row tile, then
    the lanes in order; L = 256 / min(width / 4, 64) in the vector kernel, 256 / width in the small
    one), grad_bias bitwise colsum_order32("final") of those partials and within (rows - 1) u
    sum |gh| of float64.  With y, with y and grad_bias NULL (partials only), with y NULL (gh not
    written).  y holds 0.0, -0.0, -1.0, negative and positive values.  rows 1, 31, 32, 33, 69, and
    4167 = 131 tiles (k_colsum_final's unrolled round and its remainder) at widths 12, 132, 260.
    Small kernel: widths that do not divide 256 (3, 12, 100, 127, 130, 255).  Vector kernel: 128
    (full tile, 4 rows a lane), 132 and 160 (width / 4 does not divide 256: the lanes past the
    last full row group must change nothing), 256 (8 rows a lane), 260 and 768 (further column
    tiles).  Measured ratios: the head of this file."""
    _need_gpu()
    vec = width in VEC_W
    worst = 0.0
    for rows in (1, 31, 32, 33, 69) + ((4167,) if width in (12, 132, 260) else ()):
        worst = max(worst, _act_check(bf, rows, width, vec))
    print(f"act backward width={width} {'bf16' if bf else 'f32'}: grad_bias worst ratio {worst:.3f} of (rows - 1) u sum|gh|")


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_act_backward_misaligned_takes_the_small_kernel(bf):
    """Width 128 on pointers one element off the vector alignment: the small kernel's lanes (2)."""
    _need_gpu()
    _act_check(bf, 69, 128, vec=False, off=1)


def test_act_backward_rejections():
    _need_gpu()
    gy, y = UR.act_case(33, 258)
    for bf in (False, True):
        for kw in (dict(width=258), dict(rows=0, width=12), dict(width=12, null_gh=True), dict(width=0)):
            rows, width = kw.get("rows", 33), kw["width"]
            rc, gh, gb, scratch = _act_call(bf, gy, y, rows, width, null_gh=kw.get("null_gh", False))
            assert rc == HG_ERR_ARG and gh.untouched() and gb.untouched() and scratch.untouched(), kw


# ------------------------------------------------------------------------------------------------
# hg_colsum_jobs
# ------------------------------------------------------------------------------------------------
def _colsum(jobs, njobs=None, over=None):
    """jobs: list of (src pointer, dst pointer, width, parts)."""
    n = len(jobs)
    vp = ctypes.c_void_p
    src, dst = (vp * n)(*[j[0] for j in jobs]), (vp * n)(*[j[1] for j in jobs])
    width, parts = (ctypes.c_int64 * n)(*[j[2] for j in jobs]), (ctypes.c_int * n)(*[j[3] for j in jobs])
    a = dict(src=src, dst=dst, width=width, parts=parts)
    a.update(over or {})
    rc = _lib().hg_colsum_jobs(a["src"], a["dst"], a["width"], a["parts"], n if njobs is None else njobs, _stream())
    torch.cuda.synchronize()
    return rc


def test_colsum_jobs():
    """One launch of 16 jobs over every path, each bitwise the stated order's replay and within
    (parts - 1) u sum |partials| of float64: narrow with 1, 16 (sequential) and 17, 130, 131 parts
    (k_colsum_final's order); wide (4096 columns, aligned) with 1, 2, 16 parts (sequential) and 17,
    64, 70 parts (part p into accumulator p % 8: the 8-load round at 64, round and remainder at
    70); 4098 columns and 4096 columns one float off alignment: the narrow path.  A second launch:
    a job with more than 16 parts gives the bits of hg_mlp_act_backward's own grad_bias on the
    same partials."""
    _need_gpu()
    assert len(UR.COLSUM_JOBS) == 16
    P = [UR.colsum_case(parts, width) for parts, width, _, _ in UR.COLSUM_JOBS]
    srcs = [_dev(p, off) for p, (_, _, _, off) in zip(P, UR.COLSUM_JOBS)]
    dsts = [Flat(width, guard=32) for _, width, _, _ in UR.COLSUM_JOBS]
    rc = _colsum([(s[0], d.ptr, w, p) for s, d, (p, w, _, _) in zip(srcs, dsts, UR.COLSUM_JOBS)])
    assert rc == 0
    worst, wrong = 0.0, []
    for part, d, job in zip(P, dsts, UR.COLSUM_JOBS):
        got = d.np()
        if not _same_bits(got, UR.colsum_order32(part, job[2])):
            wrong.append(job)
        p64 = part.astype(np.float64)
        worst = max(worst, _ratio(np.abs(got - p64.sum(0)), max(job[0] - 1, 0) * U24 * np.abs(p64).sum(0)))
    assert not wrong, f"jobs (parts, width, order, offset) off their stated order: {wrong}"
    print(f"colsum jobs: worst ratio {worst:.3f} of (parts - 1) u sum|partials|")
    # the header's claim: parts > 16 on a narrow job == hg_mlp_act_backward's own final reduction
    rows, width = 4167, 20
    gy, _ = UR.act_case(rows, width)
    rc, _, gb, scratch = _act_call(False, gy, None, rows, width)
    assert rc == 0
    d = Flat(width, guard=32)
    assert _colsum([(scratch.ptr, d.ptr, width, -(-rows // 32))]) == 0
    assert _same_bits(d.np(), gb.np())


def test_colsum_jobs_rejections():
    """njobs = 0 is HG_OK and touches nothing; 17 jobs, a NULL entry, a zero width or zero parts are
    rejected before the launch."""
    _need_gpu()
    P = UR.colsum_case(3, 8)
    s = _dev(P)
    d = Flat(8)
    ok = (s[0], d.ptr, 8, 3)
    assert _colsum([ok], njobs=0) == 0
    assert _colsum([ok] * 17) == HG_ERR_ARG
    for bad in ((None, d.ptr, 8, 3), (s[0], None, 8, 3), (s[0], d.ptr, 0, 3), (s[0], d.ptr, 8, 0)):
        assert _colsum([ok, bad]) == HG_ERR_ARG, bad
    for k in ("src", "dst", "width", "parts"):
        assert _colsum([ok], over={k: None}) == HG_ERR_ARG, k
    assert d.untouched()
    assert _colsum([ok]) == 0 and _same_bits(d.np(), UR.colsum_order32(P, "seq"))


# ------------------------------------------------------------------------------------------------
# hg_cast_bf16_jobs
# ------------------------------------------------------------------------------------------------
def _cast(jobs, njobs=None):
    n = len(jobs)
    vp = ctypes.c_void_p
    rc = _lib().hg_cast_bf16_jobs((vp * n)(*[j[0] for j in jobs]), (vp * n)(*[j[1] for j in jobs]),
                                  (ctypes.c_int64 * n)(*[j[2] for j in jobs]), n if njobs is None else njobs, _stream())
    torch.cuda.synchronize()
    return rc


def test_cast_bf16_jobs():
    """32 jobs in one launch: counts 1, 3, 4, 1023, 1024, 1025, 4097 (the vector path needs count %
    4 == 0 and both pointers aligned; everything else is the scalar path), sources one float and
    destinations one element off alignment.  Ties to even in both directions, the largest float32
    (-> inf), inf, signed zeros, subnormals: bitwise bf16_rne; NaN stays NaN."""
    _need_gpu()
    specs = [(UR.CAST_COUNTS[j % 7], (j // 7) % 2, (j // 14) % 2) for j in range(32)]  # count, src off, dst off
    assert {(1024, 0, 0), (1024, 1, 0), (1024, 0, 1), (4, 0, 0), (4097, 0, 0), (1, 1, 1)} <= set(specs)
    X = [UR.cast_case(n, seed=j) for j, (n, _, _) in enumerate(specs)]
    srcs = [_dev(x, so) for x, (_, so, _) in zip(X, specs)]
    dsts = [Flat(n, BF16, off=do, guard=16) for n, _, do in specs]
    assert _cast([(s[0], d.ptr, n) for s, d, (n, _, _) in zip(srcs, dsts, specs)]) == 0
    seen_nan = 0
    for x, d, spec in zip(X, dsts, specs):
        got, want = d.np(), UR.bf16_rne(x)
        nan = np.isnan(x)
        assert (got[~nan] == want[~nan]).all(), spec
        assert np.isnan(UR.bf16_to_f32(got[nan])).all(), spec
        seen_nan += int(nan.sum())
    assert seen_nan > 100
    d = Flat(4, BF16)
    ok = (srcs[2][0], d.ptr, 4)
    assert _cast([ok] * 33) == HG_ERR_ARG and _cast([ok], njobs=0) == 0
    for bad in ((None, d.ptr, 4), (srcs[2][0], None, 4), (srcs[2][0], d.ptr, 0)):
        assert _cast([ok, bad]) == HG_ERR_ARG
    assert d.untouched()


# ------------------------------------------------------------------------------------------------
# hg_linear_skinny_*
# ------------------------------------------------------------------------------------------------
SK_N = [1, 2, 3, 4, 6, 8, 12, 16]
SK_ROWS_LIST = (1, 15, 16, 17, 63, 64, 65, 129)


def _sk_forward(bf, x, ld, W, b, rows, n, k=128, xoff=0, woff=0):
    L = _lib()
    xt = np.full((rows, max(ld, 128)), NAN, f32)  # a stride below k is only ever rejected
    xt[:, :128] = x
    xp = _dev(_b16(UR.bf16_rne(xt)), xoff) if bf else _dev(xt, xoff)
    Wp, bp = _dev(W, woff), _dev(b)
    y = Flat(rows * max(n, 1))
    fn = L.hg_linear_skinny_forward_bf16 if bf else L.hg_linear_skinny_forward
    rc = fn(xp[0], ld, Wp[0], bp[0], y.ptr, rows, n, k, _stream())
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", SK_N)
def test_skinny_forward(n, bf):
    """y = x W^T + b against float64 within 1e-6 (sum_k |x_k W_nk| + |b_n|), tests/test_gpu_linear.py's
    bound, for every supported n at k = 128; rows around the 16-row group and the 64-row tile;
    16400 rows (n = 12) is past the 1024-block grid cap; rows packed and of stride 132 (float32) /
    136 (bf16), the padding columns NaN.  Measured ratios: the head of this file."""
    _need_gpu()
    worst = 0.0
    for rows in SK_ROWS_LIST + ((16400,) if n == 12 else ()):
        for ld in (128, 136 if bf else 132):
            x, W, b, _ = UR.skinny_case(rows, n)
            if bf:
                x = UR.bf16_round(x)
            rc, y = _sk_forward(bf, x, ld, W, b, rows, n)
            assert rc == 0
            y64, mag = UR.skinny_fwd64(x, W, b)
            worst = max(worst, _ratio(np.abs(y.np((rows, n)) - y64), REL * mag))
    print(f"skinny forward n={n} {'bf16' if bf else 'f32'}: worst ratio {worst:.3f} of 1e-6 x magnitude")


def _sk_backward(kind, gh, h, ldh, W, rows, n, k=128, with_wb=True, with_dx=True, hoff=0, woff=0, dxoff=0):
    """kind "f32" / "bf16" (hg_linear_skinny_backward[_bf16]) / "act" (hg_linear_skinny_backward_act)."""
    L = _lib()
    bf = kind == "bf16"
    ht = np.full((rows, max(ldh, 128)), NAN, f32)  # a stride below k is only ever rejected
    ht[:, :128] = h
    hp = _dev(_b16(UR.bf16_rne(ht)), hoff) if bf else _dev(ht, hoff)
    ghp, Wp = _dev(gh), _dev(W, woff)
    tiles = -(-rows // UR.SK_ROWS)
    nn = max(n, 1)
    assert int(L.hg_linear_skinny_backward_scratch(rows, nn, 128)) == tiles * (nn * 128 + nn)
    dx = Flat(rows * 128, BF16 if bf else torch.float32, off=dxoff)
    wb = Flat(nn * 128 + nn, guard=32)
    scratch = Flat(tiles * (nn * 128 + nn))
    colpart = Flat(tiles * 128)
    if kind == "act":
        assert int(L.hg_linear_skinny_colpart_rows(rows)) == tiles
        rc = L.hg_linear_skinny_backward_act(ghp[0], hp[0], ldh, Wp[0], dx.ptr, colpart.ptr, rows, n, k, scratch.ptr,
                                             _stream())
    else:
        fn = L.hg_linear_skinny_backward_bf16 if bf else L.hg_linear_skinny_backward
        rc = fn(ghp[0], hp[0], ldh, Wp[0], dx.ptr if with_dx else None, wb.ptr if with_wb else None, rows, n, k,
                scratch.ptr, _stream())
    torch.cuda.synchronize()
    return rc, dx, wb, scratch, colpart


@pytest.mark.parametrize("n", SK_N)
def test_skinny_backward(n):
    """Per case (rows around the 64-row tile; h packed and of stride 130):
      the partials left in scratch (grad_wb NULL) against the per-tile float64 sums: dW within
        (16 + 4) u sum |gh h| (16 fused rows a wave, then the four waves), db within 64 u sum |gh|;
      grad_wb bitwise colsum_order32("final") of those partials; scratch and dx the same bits in
        both launches; dx NULL leaves dx alone;
      dx against float64 within 1e-6 sum_j |gh_j W_jc|;
      _backward_act: gh_prev bitwise elu_bwd32(dx of _backward, h); its scratch bitwise _backward's;
        colpart against the float64 column sums per 64-row tile within 1e-6 sum_rows (dx magnitude
        x ELU factor) + (16 + 4 + 2) u sum |gh_prev| (the sums, and the factor's two roundings);
      bf16: h and dx bf16, partials as above from the rounded h, dx within 1e-6 magnitude + 2^-8 |dx|
        (bf16 keeps 8 significant bits: half a unit in the last place is 2^-8 at the bottom of a binade).
    Measured ratios: the head of this file."""
    _need_gpu()
    w = dict(dW=0.0, db=0.0, dx=0.0, colpart=0.0, dx_bf16=0.0)
    nk = n * 128
    for rows in SK_ROWS_LIST:
        for ldh in (128, 130):
            x, W, _, gh = UR.skinny_case(rows, n, 130)
            h = x[:, :128]
            ref = UR.skinny_bwd64(gh, h, W)
            tiles = -(-rows // 64)
            rc, dx1, wb1, sc1, _ = _sk_backward("f32", gh, h, ldh, W, rows, n, with_wb=False)
            assert rc == 0 and wb1.untouched()
            part = sc1.np((tiles, nk + n))
            w["dW"] = max(w["dW"], _ratio(np.abs(part[:, :nk] - ref["wb"][:, :nk]), 20 * U24 * ref["wb_mag"][:, :nk]))
            w["db"] = max(w["db"], _ratio(np.abs(part[:, nk:] - ref["wb"][:, nk:]), 64 * U24 * ref["wb_mag"][:, nk:]))
            dxv = dx1.np((rows, 128))
            w["dx"] = max(w["dx"], _ratio(np.abs(dxv - ref["dx"]), REL * ref["dx_mag"]))
            rc, dx2, wb2, sc2, _ = _sk_backward("f32", gh, h, ldh, W, rows, n)
            assert rc == 0 and _same_bits(sc2.np(), sc1.np()) and _same_bits(dx2.np(), dx1.np())
            assert _same_bits(wb2.np(), UR.colsum_order32(part, "final")), "grad_wb"
            rc, dx3, wb3, sc3, _ = _sk_backward("f32", gh, h, ldh, W, rows, n, with_dx=False)
            assert rc == 0 and dx3.untouched() and _same_bits(wb3.np(), wb2.np())
            rc, ghp, _, sc4, cp = _sk_backward("act", gh, h, ldh, W, rows, n)
            assert rc == 0 and _same_bits(sc4.np(), sc1.np())
            prev = ghp.np((rows, 128))
            assert _same_bits(prev, UR.elu_bwd32(dxv, h)), "gh_prev"
            cbound = REL * ref["colpart_elem"] + 22 * U24 * ref["colpart_mag"]
            w["colpart"] = max(w["colpart"], _ratio(np.abs(cp.np((tiles, 128)) - ref["colpart"]), cbound))
            # bf16
            hb = UR.bf16_round(h)
            refb = UR.skinny_bwd64(gh, hb, W)
            rc, dxb, wbb, scb, _ = _sk_backward("bf16", gh, hb, ldh, W, rows, n)
            assert rc == 0
            pb = scb.np((tiles, nk + n))
            _ratio(np.abs(pb[:, :nk] - refb["wb"][:, :nk]), 20 * U24 * refb["wb_mag"][:, :nk])
            _ratio(np.abs(pb[:, nk:] - refb["wb"][:, nk:]), 64 * U24 * refb["wb_mag"][:, nk:])
            assert _same_bits(wbb.np(), UR.colsum_order32(pb, "final"))
            dxf = UR.bf16_to_f32(dxb.np((rows, 128)))
            w["dx_bf16"] = max(w["dx_bf16"], _ratio(np.abs(dxf - refb["dx"]),
                                                    REL * refb["dx_mag"] + 2.0 ** -8 * np.abs(refb["dx"])))
    print(f"skinny backward n={n}: worst ratios " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


def test_skinny_rejections():
    """Unsupported n (5, 17), k != 128, a stride below k, an odd ldh, ldx % 4 != 0, misaligned x, W, h
    and dx: HG_ERR_ARG before any launch, outputs untouched."""
    _need_gpu()
    rows = 17
    x, W, b, gh = UR.skinny_case(rows, 12, 136)
    h = x[:, :128]
    W17 = np.zeros((17, 128), f32)
    for kw in (dict(n=5), dict(n=17), dict(k=64), dict(ld=124), dict(ld=130), dict(xoff=1), dict(woff=1)):
        n = kw.get("n", 12)
        rc, y = _sk_forward(False, h, kw.get("ld", 132), W17, np.zeros(17, f32), rows, n, kw.get("k", 128),
                            kw.get("xoff", 0), kw.get("woff", 0))
        assert rc == HG_ERR_ARG and y.untouched(), kw
    rc, y = _sk_forward(True, UR.bf16_round(h), 132, W, b, rows, 12)  # bf16 rows: ldx % 8
    assert rc == HG_ERR_ARG and y.untouched()
    gh17 = np.zeros((rows, 17), f32)
    for kind in ("f32", "act"):
        for kw in (dict(n=5), dict(n=17), dict(k=64), dict(ldh=126), dict(ldh=129), dict(hoff=1), dict(woff=1), dict(dxoff=1)):
            n = kw.get("n", 12)
            rc, dx, wb, scratch, cp = _sk_backward(kind, gh17[:, :n], h, kw.get("ldh", 130), W17[:n], rows, n,
                                                   kw.get("k", 128), hoff=kw.get("hoff", 0), woff=kw.get("woff", 0),
                                                   dxoff=kw.get("dxoff", 0))
            assert rc == HG_ERR_ARG and dx.untouched() and wb.untouched() and scratch.untouched() and cp.untouched(), (kind, kw)


# ------------------------------------------------------------------------------------------------
# hg_gae_scan / hg_gae_normalize through the ABI
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", [(1, 1), (3, 257), (2, 256)])
def test_gae_scan_abi(T, N):
    """Returns and raw advantages bitwise envlogic_ref.gae; stats[0..1] against the float64 sums of
    the device's raw advantages (T N 2^-53 of the magnitude sums); zero_stats = 0 adds a second call's
    sums; stats guarded at hg_gae_stats_len(N); stats_len one short returns 1 and writes nothing."""
    _need_gpu()
    L = _lib()
    rng = np.random.default_rng([T, N])
    r, v = rng.standard_normal((T, N)).astype(f32), rng.standard_normal((T, N)).astype(f32)
    dn = (rng.random((T, N)) < 0.2).astype(np.uint8)
    last = rng.standard_normal(N).astype(f32)
    d = [_dev(a) for a in (r, dn, v, last)]
    slen = int(L.hg_gae_stats_len(N))
    assert slen == 2 + 2 * -(-N // 256)
    gamma, lam = 0.994, 0.9

    def run(stats, zero, slen_=slen):
        ret, adv = Flat(T * N), Flat(T * N)
        rc = L.hg_gae_scan(d[0][0], d[1][0], d[2][0], d[3][0], ret.ptr, adv.ptr, stats.ptr, slen_, T, N, gamma, lam, zero,
                           _stream())
        torch.cuda.synchronize()
        return rc, ret, adv

    stats = Flat(2 * slen, guard=8)
    rc, ret, adv = run(stats, 1)
    assert rc == 0
    want_ret, want_adv = E.gae(r, dn, v, last, gamma, lam, normalize=False)
    assert _same_bits(ret.np((T, N)), want_ret) and _same_bits(adv.np((T, N)), want_adv)
    a64 = adv.np().astype(np.float64)
    s = stats.f64()
    eps = T * N * 2.0 ** -53
    assert abs(s[0] - a64.sum()) <= eps * np.abs(a64).sum() and abs(s[1] - (a64 * a64).sum()) <= eps * (a64 * a64).sum()
    rc, _, _ = run(stats, 0)
    s2 = stats.f64()
    assert rc == 0 and s2[0] == s[0] + s[0] and s2[1] == s[1] + s[1]
    short = Flat(2 * slen, guard=8)
    rc, ret, adv = run(short, 1, slen - 1)
    assert rc == 1 and ret.untouched() and adv.untouched() and short.untouched()


@pytest.mark.parametrize("n", [1, 3, 5, 2048 * 256 * 4 + 5])
def test_gae_normalize_abi(n):
    """Bitwise gae_norm32 from the same float64 stats: count = n_local, and count = 2 n_local with
    doubled stats (two ranks holding the same data); 2048 x 256 x 4 + 5 elements wrap the grid
    stride and leave a scalar tail; constant advantages give exactly 0."""
    _need_gpu()
    L = _lib()
    rng = np.random.default_rng(n)
    a = (0.3 + 2 * rng.standard_normal(n)).astype(f32)
    a64 = a.astype(np.float64)
    st = np.array([a64.sum(), (a64 * a64).sum()])
    for count, stats in ((n, st), (2 * n, 2 * st)):
        if count < 2:
            continue
        adv = Flat(n, fill=a)
        sp = _dev(stats.view(f32))
        assert L.hg_gae_normalize(adv.ptr, sp[0], count, n, _stream()) == 0
        torch.cuda.synchronize()
        assert _same_bits(adv.np(), UR.gae_norm32(a, stats, count)), count
    c = np.full(n, f32(1.25))
    adv = Flat(n, fill=c)
    sp = _dev(np.array([2 * n * 1.25, 2 * n * 1.25 ** 2]).view(f32))
    assert L.hg_gae_normalize(adv.ptr, sp[0], 2 * n, n, _stream()) == 0
    torch.cuda.synchronize()
    assert (adv.np() == 0).all()
    if n == 5:
        ok = Flat(8, fill=np.ones(8, f32))
        off = Flat(8, off=1, fill=np.ones(8, f32))
        assert L.hg_gae_normalize(off.ptr, sp[0], 10, 5, _stream()) == 1
        assert L.hg_gae_normalize(ok.ptr, sp[0], 1, 5, _stream()) == 1
        assert L.hg_gae_normalize(ok.ptr, None, 10, 5, _stream()) == 1 and L.hg_gae_normalize(ok.ptr, sp[0], 10, 0, _stream()) == 1
        torch.cuda.synchronize()
        assert (ok.np() == 1).all() and (off.np() == 1).all()
