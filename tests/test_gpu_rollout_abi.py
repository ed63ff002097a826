"""csrc/hg_rollout.hip through its C ABI (humanoid._native), against the replayed numpy references of
oracle/rollout_ref.py, at the smallest shapes that reach every branch of the kernels.

  hg_rollout_act / _act_head / _act_tail   noise replayed from the Philox key (seed, env + row_offset,
      counter, block, purpose 9) and held to float64 Box-Muller; log-prob to float64 on the stored
      a / mu / sigma; mu / sigma / value / observation rows bitwise; the fused head and tail bitwise
      against their two-launch forms and to float64; argument rejections
  hg_rollout_env                           the time-out bootstrap and its NULL arguments
  hg_gather_rows / _ex                     both paths (every table <= 1024 wide and 4-byte, or not)
  hg_gather_stacked                        the frame-stack rebuild against the deque stepped literally

What would fail if the kernel were wrong (each checked once against a deliberately altered build):
  a wrong Box-Muller lane, a dropped row_offset, a lost counter high word
                                   -> test_act_noise_replayed (A >= 3; row_offset 4096; counter 2^32 + 5)
  the A > 16 one-thread-per-env branch (its z4 refill)   -> test_act_noise_replayed[17], [64]
  the copy waves' second grid-stride pass                -> test_act_copy_wraps_the_wave_cap
  a dropped or wrong log-prob term                       -> check_logp, in every act / head / tail case
  the fused tail off its one tested shape                -> test_act_tail (tail_k 4 / 36 / 96 / 256)
  the frame-stack rebuild (reset window, init splice, passes, dtypes, layouts) -> test_gather_stacked
  the 1024-wide path split of the row gather             -> test_gather_rows
  hg_rollout_env and its NULL arguments                  -> test_rollout_env

Every output is allocated with guard rows (and guard columns where the ABI takes a row stride),
prefilled with a NaN-pattern sentinel that must be intact afterwards.  Rejections are tested only
where the entry point returns HG_ERR_ARG before any launch."""
import ctypes
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_REPO, "humanoid-gym-with-comments_amd"), os.path.join(_REPO, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rollout_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HG_ERR_ARG = 1
F32, F16, BF16 = 0, 1, 2  # HG_DTYPE_*
TDT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
SENT = {4: 0x7FA5A5A5, 2: 0x7DA5, 1: 0xA5}  # NaN bit patterns (fp32, fp16 / bf16), a byte
IDT = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
SEEDS = (0x9E3779B97F4A7C15, 0x0123456700000005)  # non-zero high words
BIG = (1 << 32) + 5
REL = 1e-6  # tests/test_gpu_linear.py's stated bound for the f32 matrix-core linear layers
U23, U24 = 2.0 ** -23, 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from humanoid import _native as N
    return N.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)  # a copy: shared references stay read-only


class Guarded:
    """A rows x width output (row stride ld) with guard rows below and guard columns up to ld, all
    prefilled with the sentinel; bits() checks the guards and returns the payload as integers."""

    def __init__(self, rows, width, dtype=torch.float32, ld=None, guard_rows=3):
        self.rows, self.width, self.ld, self.dtype = rows, width, ld or width, dtype
        self.es = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((rows + guard_rows, self.ld), SENT[self.es], dtype=IDT[self.es], device=DEV)

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def bits(self):
        host = self.raw.cpu()
        keep = torch.ones_like(host, dtype=torch.bool)
        keep[:self.rows, :self.width] = False
        assert bool((host[keep] == SENT[self.es]).all()), "a guard row or column was overwritten"
        return host[:self.rows, :self.width].contiguous()

    def get(self):
        return self.bits().view(self.dtype)

    def np(self):
        return self.get().numpy()

    def untouched(self):
        return bool((self.raw == SENT[self.es]).all().item())


def _bits(t):
    """integer view of a CPU tensor / numpy array, for bitwise comparison (NaN-safe, -0 != +0)."""
    t = torch.from_numpy(np.array(t, order="C")) if isinstance(t, np.ndarray) else t.contiguous()
    return t.view(IDT[t.element_size()])


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool((a == b).all())


# ------------------------------------------------------------------------------------------------
# hg_rollout_act / _act_head / _act_tail
# ------------------------------------------------------------------------------------------------
ACT_NAMES = ["mean", "std", "value", "obs", "critic_obs", "num_envs", "num_actions", "obs_width",
             "critic_obs_width", "obs_ld", "obs_col0", "critic_obs_ld", "actions_out", "logp_out", "mu_out",
             "sigma_out", "value_out", "obs_out", "obs_out_ld", "critic_obs_out", "obs_fp16", "row_offset", "seed",
             "counter", "stream"]
HEAD_NAMES = ["h", "h_ld", "W", "b", "head_k"] + ACT_NAMES[1:]
TAIL_NAMES = ["x", "x_ld", "W3", "b3", "tail_k", "W", "b"] + ACT_NAMES[1:]
OUT_KEYS = ("actions", "logp", "mu", "sigma", "value", "obs", "cobs")
# fp16 rounding edges: the largest finite value, just below / exactly at the overflow tie (65520 ->
# inf by round-to-nearest-even), just above / below half the smallest subnormal, signed zeros
FP16_EDGES = np.array([65504.0, 65519.996, 65520.0, 6e-8, 2.98e-8, -0.0, 1e-10, -1e-10, -65519.996, -65520.0],
                      np.float32)


class ActCase:
    """Inputs of one policy step, on the host and on the device; run() allocates fresh guarded outputs,
    launches one of the three entry points and returns the outputs as numpy / torch CPU arrays."""

    def __init__(self, n, A, obs_w=5, *, obs_c0=0, cobs_w=0, obs_out_ld=0, fp16=False, row_offset=0,
                 seed=SEEDS[0], counter=0, mean=None, std=None, with_value=True, edges=False, rng_seed=0):
        rng = np.random.default_rng([rng_seed, n, A, obs_w])
        self.n, self.A, self.obs_w, self.obs_c0, self.cobs_w = n, A, obs_w, obs_c0, cobs_w
        self.obs_out_ld, self.fp16, self.row_offset, self.seed, self.counter = obs_out_ld, fp16, row_offset, seed, counter
        self.mean = rng.standard_normal((n, A)).astype(np.float32) if mean is None else np.asarray(mean, np.float32)
        self.std = (0.3 + rng.random(A)).astype(np.float32) if std is None else np.asarray(std, np.float32)
        self.value = rng.standard_normal(n).astype(np.float32) if with_value else None
        self.obs_ld = obs_c0 + obs_w + 3
        self.obs = (3 * rng.standard_normal((n, self.obs_ld))).astype(np.float32)
        self.cobs_ld = cobs_w + 2
        self.cobs = (3 * rng.standard_normal((n, self.cobs_ld))).astype(np.float32) if cobs_w else None
        if edges:
            for x in (self.obs, self.cobs):
                if x is not None:
                    v = x.reshape(-1)[::3]
                    v[:] = np.resize(FP16_EDGES, v.shape)
        self.d = {k: _dev(getattr(self, k)) for k in ("mean", "std", "value", "obs", "cobs")
                  if getattr(self, k) is not None}
        self.extra = {}

    def set_head(self, h_ld=128, rng_seed=1):
        rng = np.random.default_rng([rng_seed, self.n])
        self.h = rng.standard_normal((self.n, h_ld)).astype(np.float32)
        self.W = (rng.standard_normal((12, 128)) / 128 ** 0.5).astype(np.float32)
        self.b = (0.1 * rng.standard_normal(12)).astype(np.float32)
        self.d.update(h=_dev(self.h), W=_dev(self.W), b=_dev(self.b))
        self.extra.update(h=self.d["h"].data_ptr(), h_ld=h_ld, W=self.d["W"].data_ptr(), b=self.d["b"].data_ptr(),
                          head_k=128)
        return self

    def set_tail(self, tail_k, x_ld, rng_seed=2):
        rng = np.random.default_rng([rng_seed, self.n, tail_k])
        self.x = rng.standard_normal((self.n, x_ld)).astype(np.float32)
        self.W3 = (rng.standard_normal((128, tail_k)) / tail_k ** 0.5).astype(np.float32)
        self.b3 = (0.1 * rng.standard_normal(128)).astype(np.float32)
        self.tail_k = tail_k
        self.d.update(x=_dev(self.x), W3=_dev(self.W3), b3=_dev(self.b3))
        self.extra.update(x=self.d["x"].data_ptr(), x_ld=x_ld, W3=self.d["W3"].data_ptr(),
                          b3=self.d["b3"].data_ptr(), tail_k=tail_k)
        return self

    def outputs(self):
        n, A, dt = self.n, self.A, torch.float16 if self.fp16 else torch.float32
        g = {"actions": Guarded(n, A), "logp": Guarded(n, 1), "mu": Guarded(n, A), "sigma": Guarded(n, A),
             "value": Guarded(n, 1), "obs": Guarded(n, self.obs_w, dt, ld=self.obs_out_ld or self.obs_w)}
        if self.cobs_w:
            g["cobs"] = Guarded(n, self.cobs_w, dt)
        return g

    def args(self, g):
        p = lambda k: self.d[k].data_ptr() if k in self.d else None  # noqa: E731
        a = dict(mean=p("mean"), std=p("std"), value=p("value"), obs=p("obs"), critic_obs=p("cobs"), num_envs=self.n,
                 num_actions=self.A, obs_width=self.obs_w, critic_obs_width=self.cobs_w, obs_ld=self.obs_ld,
                 obs_col0=self.obs_c0, critic_obs_ld=self.cobs_ld, actions_out=g["actions"].ptr,
                 logp_out=g["logp"].ptr, mu_out=g["mu"].ptr, sigma_out=g["sigma"].ptr, value_out=g["value"].ptr,
                 obs_out=g["obs"].ptr, obs_out_ld=self.obs_out_ld, critic_obs_out=g["cobs"].ptr if "cobs" in g else None,
                 obs_fp16=int(self.fp16), row_offset=self.row_offset, seed=self.seed, counter=self.counter,
                 stream=_stream())
        a.update(self.extra)
        return a

    def call(self, kind, g, **over):
        L = _lib()
        fn, names = {"act": (L.hg_rollout_act, ACT_NAMES), "head": (L.hg_rollout_act_head, HEAD_NAMES),
                     "tail": (L.hg_rollout_act_tail, TAIL_NAMES)}[kind]
        a = self.args(g)
        a.update(over)
        return fn(*[a[k] for k in names])

    def run(self, kind, **over):
        g = self.outputs()
        rc = self.call(kind, g, **over)
        assert rc == 0, (kind, rc)
        torch.cuda.synchronize()
        o = {k: v.get() for k, v in g.items() if k != "value"}
        if self.value is None:
            assert g["value"].untouched(), "value == NULL (deferred values) must leave value_out alone"
        else:
            o["value"] = g["value"].get()
        return o

    # --- the parts every launch must get bitwise: value, sigma, the observation rows ---
    def check_copies(self, o):
        assert _same_bits(o["sigma"], np.broadcast_to(self.std, (self.n, self.A)))
        if self.value is not None:
            assert _same_bits(o["value"], self.value[:, None])
        dt = np.float16 if self.fp16 else np.float32
        with np.errstate(over="ignore"):
            want = self.obs[:, self.obs_c0:self.obs_c0 + self.obs_w].astype(dt)
            assert _same_bits(o["obs"], want), "observation rows"
            if self.cobs_w:
                assert _same_bits(o["cobs"], self.cobs[:, :self.cobs_w].astype(dt)), "critic rows"

    def check_logp(self, o):
        """log-prob against float64 on the stored a / mu / sigma: (A + 8) 2^-24 S per row, no floor.
        Returns the worst ratio to the bound."""
        lp, S = RR.log_prob64(o["actions"].numpy(), o["mu"].numpy(), o["sigma"].numpy())
        err = np.abs(o["logp"].numpy()[:, 0].astype(np.float64) - lp)
        bound = (self.A + 8) * U24 * S
        assert (err <= bound).all(), f"log-prob: worst ratio {(err / bound).max():.3f}"
        return float((err / bound).max())

    def check_noise(self, o):
        """the stored actions against mu + sigma z64 of the replayed draws, on the stored mu / sigma:
        s 4 2^-23 r + 2^-24 |s z| + 2^-24 |a| (the noise bound, the product and the sum roundings)."""
        z64, r = RR.act_normals64(self.seed, self.row_offset, self.counter, self.n, self.A)
        s, a, m = (o[k].numpy().astype(np.float64) for k in ("sigma", "actions", "mu"))
        err, bound = np.abs(a - (m + s * z64)), s * 4 * U23 * r + U24 * np.abs(s * z64) + U24 * np.abs(a)
        assert (err <= bound).all(), f"actions: worst ratio {(err / bound).max():.3f}"


def _noise_units(a_over_s, z64, r):
    """max |z_gpu - z64| in units of 2^-23 r (asserted <= 4)."""
    err = np.abs(a_over_s.astype(np.float64) - z64)
    assert (err <= 4 * U23 * r).all(), f"noise: {np.max(err[r > 0] / (U23 * r[r > 0])):.3f} x 2^-23 r"
    return float(np.max(err[r > 0] / (U23 * r[r > 0]))) if (r > 0).any() else 0.0


@pytest.mark.parametrize("A", [1, 3, 12, 16, 17, 64])
def test_act_noise_replayed(A):
    """hg_rollout_act's noise is philox_key(seed, e + row_offset, counter, j >> 2) -> normals4 lane
    j & 3: with mean 0 and a power-of-two std the stored action IS z times an exact scale, held to
    the float64 Box-Muller of the same draws within 4 * 2^-23 * r (r the draw's radius): logf <= 1
    ulp halved by the square root, sqrtf <= 1 ulp, sincosf <= 2 ulp, one product rounding.
    A <= 16 is the 16-lanes-per-env path, A in {17, 64} the one-thread-per-env path with the z4
    refill; row_offset 4096 and the counter 2^32 + 5 would be other numbers if the offset or the
    counter's high word were dropped (tests/test_rollout_ref.py::test_inputs_discriminate).
    Measured on MI355X: max 1.436 x 2^-23 r over every case (1.121 at A <= 3; the numpy float32
    oracle is at 1.55 of float64 on its own draws); log-prob worst ratio 0.320 of its bound (A = 1).

    General mean / std: a against m + s z64 within s 4 2^-23 r + 2^-24 |s z| + 2^-24 |a| (the
    product and sum roundings: one or two, contraction allowed).  mu, sigma, value and the
    observation / critic rows bitwise; value == NULL leaves value_out untouched."""
    _need_gpu()
    worst, worst_lp = 0.0, 0.0
    pow2 = np.resize(np.array([0.5, 2.0, 1.0], np.float32), A)
    for n in (1, 15, 16, 17, 257):
        for i, (off, ctr) in enumerate(itertools.product((0, 4096), (0, 7, BIG))):
            seed = SEEDS[i % 2]
            z64, r = RR.act_normals64(seed, off, ctr, n, A)
            kw = dict(obs_w=5, obs_c0=2 * (i % 2), cobs_w=3 * (i % 2), row_offset=off, seed=seed, counter=ctr,
                      with_value=i % 3 != 1, fp16=i % 4 == 3)
            # mean 0, std 1
            c = ActCase(n, A, mean=np.zeros((n, A)), std=np.ones(A), **kw)
            o1 = c.run("act")
            c.check_copies(o1)
            assert _same_bits(o1["mu"], c.mean)
            worst = max(worst, _noise_units(o1["actions"].numpy(), z64, r))
            worst_lp = max(worst_lp, c.check_logp(o1))
            # mean 0, std 0.5 / 2 / 1 by action: the same z, scaled exactly
            c = ActCase(n, A, mean=np.zeros((n, A)), std=pow2, **kw)
            o2 = c.run("act")
            c.check_copies(o2)
            assert _same_bits(o2["actions"].numpy() / pow2, o1["actions"])
            worst_lp = max(worst_lp, c.check_logp(o2))
            # random mean, std in [0.3, 1.3]
            c = ActCase(n, A, **kw)
            o3 = c.run("act")
            c.check_copies(o3)
            assert _same_bits(o3["mu"], c.mean)
            c.check_noise(o3)
            worst_lp = max(worst_lp, c.check_logp(o3))
    print(f"A={A}: noise max {worst:.3f} x 2^-23 r (bound 4); log-prob worst ratio {worst_lp:.3f} of (A+8) 2^-24 S")


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("w", [1, 64, 65, 192, 193, 256, 257, 449, 705])
def test_act_observation_copy(w, fp16):
    """The observation rows of the slot: a column range [obs_col0, obs_col0 + w) of strided source
    rows into rows of stride obs_out_ld (0: packed; the frame-only storage passes T W), fp32 or
    fp16 (bitwise numpy's round-to-nearest-even astype, overflow and subnormal edges included),
    with and without the critic table; widths around the 64-lane and 4 x 64 unroll boundaries."""
    _need_gpu()
    for c0, pad, cw in itertools.product((0, 11), (0, 7), (0, 219)):
        c = ActCase(6, 3, obs_w=w, obs_c0=c0, cobs_w=cw, obs_out_ld=(w + pad) if pad else 0, fp16=fp16, edges=True,
                    seed=SEEDS[1], counter=3)
        assert c.obs_ld > c0 + w
        o = c.run("act")
        c.check_copies(o)
        c.check_logp(o)


@pytest.mark.parametrize("fp16", [False, True])
@pytest.mark.parametrize("kind", ["act", "head", "tail"])
def test_act_copy_wraps_the_wave_cap(kind, fp16):
    """n = 4100 with a critic table is 8200 copy rows: past the 2048 blocks x 4 waves of k_act and
    the 1024 blocks x 8 waves of k_act_tail, so the copy waves take a second grid-stride pass (as
    they do on every step at 8192 envs per rank).  Every row bitwise, the noise replayed."""
    _need_gpu()
    n = 4100
    c = ActCase(n, 12, obs_w=5, obs_c0=1, cobs_w=3, fp16=fp16, edges=True, row_offset=4096, seed=SEEDS[1], counter=BIG)
    c.set_head().set_tail(36, 40)
    o = c.run(kind)
    c.check_copies(o)
    c.check_logp(o)
    c.check_noise(o)


def _head_bound(h, W, b):
    h, W, b = h.astype(np.float64), W.astype(np.float64), b.astype(np.float64)
    return h @ W.T + b, np.abs(h) @ np.abs(W).T + np.abs(b)


@pytest.mark.parametrize("h_ld", [128, 132])
@pytest.mark.parametrize("n", [1, 17, 257])
def test_act_head(n, h_ld):
    """hg_rollout_act_head: mu against the float64 W h + b within (128 + 1) 2^-24 (sum |h W| + |b|)
    (128 products and additions in some order, then the bias), and every output bitwise equal to
    hg_linear_skinny_forward followed by hg_rollout_act on the same seed / offset / counter."""
    _need_gpu()
    c = ActCase(n, 12, obs_w=7, obs_c0=1, cobs_w=4, row_offset=4096, seed=SEEDS[1], counter=BIG).set_head(h_ld)
    o = c.run("head")
    c.check_copies(o)
    c.check_logp(o)
    mu64, mag = _head_bound(c.h[:, :128], c.W, c.b)
    err = np.abs(o["mu"].numpy().astype(np.float64) - mu64)
    assert (err <= 129 * U24 * mag).all(), f"head: worst ratio {(err / (129 * U24 * mag)).max():.3f}"
    print(f"head n={n} h_ld={h_ld}: worst {(err / (129 * U24 * mag)).max():.3f} of 129 x 2^-24 x magnitude; "
          f"{(err / (REL * mag)).max():.3f} of test_gpu_linear's REL = 1e-6")
    y = Guarded(n, 12)
    rc = _lib().hg_linear_skinny_forward(c.d["h"].data_ptr(), h_ld, c.d["W"].data_ptr(), c.d["b"].data_ptr(), y.ptr,
                                         n, 12, 128, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _same_bits(y.get(), o["mu"])
    two = c.run("act", mean=y.ptr)
    for k in o:
        assert _same_bits(o[k], two[k]), k
    c.check_noise(o)


@pytest.mark.parametrize("tail_k", [4, 36, 96, 256])
def test_act_tail(tail_k):
    """hg_rollout_act_tail at tail_k below one 32-wide chunk, with a partial last chunk (36), a
    multiple of 32 that is no multiple of 64 (96: the two-chunk pipeline's odd end) and the
    product's 256; rows packed and strided; n = 1, one block and a row, two blocks and a row.
    Bitwise hg_linear_act_forward(act = 1, tile = 5) followed by hg_rollout_act_head; the hidden
    row to the float64 ELU within test_gpu_linear's bound, mu to float64 from that row."""
    _need_gpu()
    L = _lib()
    for n, pad in itertools.product((1, 17, 33), (0, 4)):
        c = ActCase(n, 12, obs_w=7, obs_c0=1, cobs_w=4, row_offset=4096, seed=SEEDS[0], counter=7)
        c.set_head().set_tail(tail_k, tail_k + pad)
        o = c.run("tail")
        c.check_copies(o)
        c.check_logp(o)
        c.check_noise(o)
        y = Guarded(n, 128)
        rc = L.hg_linear_act_forward(c.d["x"].data_ptr(), tail_k + pad, c.d["W3"].data_ptr(), c.d["b3"].data_ptr(),
                                     y.ptr, 128, n, 128, tail_k, 1, 5, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        hid = y.np()
        pre, mag = _head_bound(c.x[:, :tail_k], c.W3, c.b3)
        elu64 = np.where(pre > 0, pre, np.expm1(pre))
        err = np.abs(hid.astype(np.float64) - elu64)
        assert (err <= REL * mag).all(), f"hidden row: worst ratio {(err / (REL * mag)).max():.3f}"
        two = c.run("head", h=y.ptr, h_ld=128)
        for k in o:
            assert _same_bits(o[k], two[k]), (k, n, pad)
        mu64, mag2 = _head_bound(hid, c.W, c.b)
        err2 = np.abs(o["mu"].numpy().astype(np.float64) - mu64)
        assert (err2 <= 129 * U24 * mag2).all()
        print(f"tail k={tail_k} n={n} x_ld={tail_k + pad}: hidden worst {(err / (REL * mag)).max():.3f} of REL x "
              f"magnitude; mu worst {(err2 / (129 * U24 * mag2)).max():.3f} of 129 x 2^-24 x magnitude")


def test_act_rejections():
    """Every argument check of the three entry points returns HG_ERR_ARG before any launch: the
    outputs keep their sentinels."""
    _need_gpu()
    c = ActCase(5, 12, obs_w=7, obs_c0=2, cobs_w=4, obs_out_ld=9).set_head().set_tail(8, 8)
    bad_shape = [dict(obs_ld=c.obs_c0 + c.obs_w - 1), dict(obs_out_ld=c.obs_w - 1), dict(critic_obs_ld=c.cobs_w - 1)]
    cases = [("act", o) for o in [dict(num_actions=0), dict(num_actions=65), dict(mean=None)] + bad_shape]
    cases += [("head", o) for o in [dict(num_actions=0), dict(num_actions=65), dict(num_actions=11),
                                    dict(num_actions=16), dict(head_k=64), dict(head_k=256)] + bad_shape]
    cases += [("tail", o) for o in [dict(num_actions=0), dict(num_actions=65), dict(num_actions=11),
                                    dict(num_actions=16), dict(tail_k=6), dict(tail_k=7, x_ld=8)] + bad_shape]
    for kind, over in cases:
        g = c.outputs()
        rc = c.call(kind, g, **over)
        torch.cuda.synchronize()
        assert rc == HG_ERR_ARG, (kind, over, rc)
        for k, v in g.items():
            assert v.untouched(), (kind, over, k)
    for kind in ("act", "head", "tail"):  # the unmodified arguments are valid
        c.check_copies(c.run(kind))


# ------------------------------------------------------------------------------------------------
# hg_rollout_env
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rollout_env(n):
    """rewards[t] = r + gamma V time_out: bitwise r where the env did not time out, elsewhere within
    2^-24 |gamma V| + 2^-24 |result| of float64 (one or two roundings); dones and time-outs
    bitwise; values == NULL defers the bootstrap (rewards bitwise r, time-outs kept), time_outs ==
    NULL writes zero time-outs, time_outs_out == NULL changes nothing else."""
    _need_gpu()
    L = _lib()
    rng = np.random.default_rng(n)
    r = rng.standard_normal(n).astype(np.float32)
    v = (5 * rng.standard_normal(n)).astype(np.float32)
    reset = (rng.random(n) < 0.3).astype(np.uint8)
    to = (rng.random(n) < 0.5).astype(np.uint8)
    if n > 1:
        to[0], to[1] = 0, 1
    gamma = 0.994
    d = {k: _dev(x) for k, x in dict(r=r, v=v, reset=reset, to=to).items()}

    def run(values=True, time_outs=True, time_outs_out=True):
        g = {"rew": Guarded(n, 1), "dones": Guarded(n, 1, torch.uint8), "to": Guarded(n, 1, torch.uint8)}
        rc = L.hg_rollout_env(d["r"].data_ptr(), d["reset"].data_ptr(), d["to"].data_ptr() if time_outs else None,
                              d["v"].data_ptr() if values else None, n, gamma, g["rew"].ptr, g["dones"].ptr,
                              g["to"].ptr if time_outs_out else None, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        if not time_outs_out:
            assert g["to"].untouched()
        return {k: x.np()[:, 0] for k, x in g.items() if k != "to" or time_outs_out}

    o = run()
    assert np.array_equal(o["dones"], reset) and np.array_equal(o["to"], to)
    assert _same_bits(o["rew"][to == 0], r[to == 0])
    want = RR.bootstrap64(r, v, to, gamma)
    gv = np.abs(float(np.float32(gamma)) * v.astype(np.float64))
    err = np.abs(o["rew"].astype(np.float64) - want)
    bound = U24 * gv + U24 * np.abs(o["rew"].astype(np.float64))
    assert (err[to == 1] <= bound[to == 1]).all(), f"bootstrap: worst ratio {(err / bound)[to == 1].max():.3f}"
    if (to == 1).any():
        print(f"env n={n}: bootstrap worst ratio {(err / bound)[to == 1].max():.3f}")
        assert not _same_bits(o["rew"], r)  # the bootstrap did something
    o2 = run(values=False)
    assert _same_bits(o2["rew"], r) and np.array_equal(o2["dones"], reset) and np.array_equal(o2["to"], to)
    o3 = run(time_outs=False)
    assert _same_bits(o3["rew"], r) and np.array_equal(o3["dones"], reset) and not o3["to"].any()
    o4 = run(time_outs_out=False)
    assert _same_bits(o4["rew"], o["rew"]) and np.array_equal(o4["dones"], reset)
    for bad in (dict(n=0), dict(rew=None)):  # rejected before any launch
        g = Guarded(n, 1)
        rc = L.hg_rollout_env(d["r"].data_ptr() if "rew" not in bad else None, d["reset"].data_ptr(), None, None,
                              bad.get("n", n), gamma, g.ptr, g.ptr, None, _stream())
        assert rc == HG_ERR_ARG and g.untouched()


# ------------------------------------------------------------------------------------------------
# hg_gather_rows / hg_gather_rows_ex
# ------------------------------------------------------------------------------------------------
def _table(rng, rows, w, dt, mag=1.0):
    return (mag * torch.from_numpy(rng.standard_normal((rows, w)).astype(np.float32))).to(TDT[dt])


def _gather(spec, rows, src_rows, form, rng):
    """spec: list of (width, src dtype, dst dtype, magnitude) or None (a NULL table of the six-pointer
    form).  Launches once and compares every destination bitwise with src[idx] cast by torch on the
    CPU; the guard rows must be intact."""
    from humanoid import _native as N
    L = _lib()
    idx = rng.integers(0, src_rows, rows)
    if rows >= 3:
        idx[1] = idx[0]  # duplicates
    idx_d = _dev(idx.astype(np.int64))
    src = [None if s is None else _table(rng, src_rows, s[0], s[1], s[3]) for s in spec]
    src_d = [None if t is None else t.to(DEV) for t in src]
    dst = [None if s is None else Guarded(rows, s[0], TDT[s[2]]) for s in spec]
    if form == "six":
        a = []
        for s, t, g in zip(spec, src_d, dst):
            a += [None, None, 0, 0] if s is None else [t.data_ptr(), g.ptr, s[0], t.element_size()]
        a += [None, None, 0, 0] * (3 - len(spec))
        rc = L.hg_gather_rows(idx_d.data_ptr(), rows, src_rows, *a, _stream())
    else:
        tabs = (N.GatherTable * len(spec))(*[N.GatherTable(t.data_ptr(), g.ptr, s[0], s[1], s[2])
                                             for s, t, g in zip(spec, src_d, dst)])
        rc = L.hg_gather_rows_ex(idx_d.data_ptr(), rows, src_rows, tabs, len(spec), _stream())
    assert rc == 0, (spec, rc)
    torch.cuda.synchronize()
    for s, t, g in zip(spec, src, dst):
        if s is not None:
            assert _same_bits(g.get(), t[torch.from_numpy(idx)].to(TDT[s[2]])), (s, rows, src_rows, form)


def _copy(w, dt=F32):
    return (w, dt, dt, 3.0)


@pytest.mark.parametrize("src_rows", [1, 37])
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_gather_rows(rows, src_rows):
    """Row gathers, bitwise: every table 4-byte and <= 1024 wide takes the all-loads-first path, one
    1025-wide (or 2-byte, or converting) table sends the launch down the general path.  Widths around
    the 64-lane, 256-element and 1024-element boundaries; 2-byte elements at odd widths; fp16 -> bf16
    and fp32 -> bf16 against torch's CPU cast; 1, 2 and 3 tables; a NULL middle table; rows around
    the 4 rows of a block; duplicate indices; a one-row source."""
    _need_gpu()
    rng = np.random.default_rng([rows, src_rows])
    groups = [[_copy(1), _copy(63), _copy(64)], [_copy(65), _copy(255), _copy(256)],
              [_copy(257), _copy(1024), _copy(1023)],   # short path
              [_copy(257), _copy(1025), _copy(1023)],   # the same but one table: general path
              [_copy(1, F16), _copy(63, F16), _copy(65, F16)], [_copy(255, F16), _copy(257, F16), _copy(1023, F16)],
              [_copy(1025, F16), _copy(64), _copy(1024, F16)],
              [_copy(705)], [_copy(1024)], [_copy(1025)], [_copy(219), _copy(43, F16)], [_copy(256), _copy(1024)]]
    for i, spec in enumerate(groups):
        _gather(spec, rows, src_rows, "six" if i % 2 == 0 else "ex", rng)
    _gather([_copy(65), None, _copy(1024)], rows, src_rows, "six", rng)   # NULL middle table: short path
    _gather([_copy(65), None, _copy(1025)], rows, src_rows, "six", rng)
    _gather([_copy(7, F16), None, None], rows, src_rows, "six", rng)
    for mag in (7.0, 1e-3):
        _gather([(257, F16, BF16, mag), (65, F32, BF16, mag), (1025, F32, BF16, mag)], rows, src_rows, "ex", rng)
        _gather([(63, F32, F32, mag), (1023, F16, BF16, mag), (5, BF16, BF16, mag)], rows, src_rows, "ex", rng)


def test_gather_rows_rejections():
    _need_gpu()
    from humanoid import _native as N
    L = _lib()
    src, idx, g = torch.zeros(4, 8, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV), Guarded(2, 8)
    ok = [idx.data_ptr(), 2, 4, src.data_ptr(), g.ptr, 8, 4] + [None, None, 0, 0] * 2 + [_stream()]
    for i, bad in ((0, None), (1, 0), (2, 0), (3, None), (6, 3), (5, 0), (4, None)):
        a = list(ok)
        a[i] = bad
        assert L.hg_gather_rows(*a) == HG_ERR_ARG, i
    for sd, dd in ((F32, F16), (BF16, F32), (F16, F32), (3, 3)):  # only -> bf16 conversions exist
        tabs = (N.GatherTable * 1)(N.GatherTable(src.data_ptr(), g.ptr, 8, sd, dd))
        assert L.hg_gather_rows_ex(idx.data_ptr(), 2, 4, tabs, 1, _stream()) == HG_ERR_ARG
    tabs = (N.GatherTable * 4)(*[N.GatherTable(src.data_ptr(), g.ptr, 8, F32, F32)] * 4)
    assert L.hg_gather_rows_ex(idx.data_ptr(), 2, 4, tabs, 4, _stream()) == HG_ERR_ARG
    assert L.hg_gather_rows_ex(idx.data_ptr(), 2, 4, tabs, 0, _stream()) == HG_ERR_ARG
    torch.cuda.synchronize()
    assert g.untouched()


# ------------------------------------------------------------------------------------------------
# hg_gather_stacked
# ------------------------------------------------------------------------------------------------
GEOMS = [(1, 1, 1, 1),
         (3, 5, 1, 7),      # no history
         (4, 3, 6, 5),      # every row reaches into init
         (9, 4, 3, 70),
         (5, 3, 4, 200),    # 800 elements: two passes of the f32 -> f32 path (768 per pass)
         (5, 3, 4, 300),    # 1200 elements: two passes of the other path (1024 per pass)
         (70, 2, 64, 3),    # the widest reset scan
         (30, 8, 15, 47)]   # the product's geometry
PAIRS = [(F32, F32), (F32, BF16), (F16, F16), (F16, BF16), (F16, F32)]
# plain tables gathered by the same launch: <= 256 wide and 4-byte is the early path, else the late one
PLAIN = [[], [_copy(1), _copy(256)], [_copy(4), _copy(5)], [_copy(255)], [_copy(257), _copy(705)],
         [_copy(5, F16), (7, F32, BF16, 7.0)], [_copy(256), _copy(257)]]


def _stack_dones(rng, T, N, F):
    """Random resets at p = 0.15 plus two planted envs (F > 1, T > 1): env 0 is reset by steps 0 and 1
    only, env 1 by step 0 only, up to slot F + 1 (random again after it).  Their rows give
      e  row 0 of env 0: a done at slot t itself and one after it, nothing cleared
      a  row 1: a reset at t - 1 (and, t < F - 1, inside the init-covered span: f)
      d  rows 2, 3 of env 0: two resets in the window, the later one wins
      b  row F - 1 of env 1: a reset exactly at the oldest visible slot tau
      c  row F of env 1: a reset at tau - 1, which must not zero anything."""
    dones = (rng.random((T, N)) < 0.15).astype(np.uint8)
    if F > 1 and T > 1:
        dones[:F + 2, :2] = 0
        dones[0, :2] = 1
        dones[1, 0] = 1
    return dones


def _stack_kinds(ref, dones, T, N, F, W):
    """Which planted kinds the REFERENCE rows show: nz = the leading all-zero frames of the row as
    stack_replay built it, classified by the resets that produced it."""
    kinds = set()
    for t in range(T):
        for e in range(N):
            row = ref[t, e].reshape(F, W)
            zero = (row == 0).all(1)
            assert ((row == 0).any(1) == zero).all()  # frames are never partly zero (inputs are non-zero)
            nz = int(np.argmin(zero)) if not zero.all() else F
            assert not zero[nz:].any() and nz <= F - 1
            tau = t - (F - 1)
            win = [r for r in range(max(tau, 0), t) if dones[r, e]]
            if win and win[-1] == t - 1 and nz == F - 1:
                kinds.add("a")
            if tau >= 0 and win == [tau] and nz == 1 and F > 2:
                kinds.add("b")
            if tau >= 1 and dones[tau - 1, e] and not win and nz == 0:
                kinds.add("c")
            if len(win) >= 2 and nz == win[-1] - tau + 1:
                kinds.add("d")
                if win[-1] < t - 1:
                    kinds.add("d2")
            if dones[t, e] and (t + 1 >= T or dones[t + 1, e]) and not win and nz == 0:
                kinds.add("e")
            if t < F - 1 and win and nz == win[-1] - tau + 1 and nz > F - 1 - t:
                kinds.add("f")
    return kinds


def _stack_required(T, N, F, W):
    if F == 1 or T == 1:
        return set()
    need = {"a", "d", "e", "f"}
    if T >= F and F > 2:
        need.add("b")
    if T >= F + 1:
        need.add("c")
    if F >= 4 and T >= 4:
        need.add("d2")
    return need


@functools.lru_cache(maxsize=None)
def _stack_case(geom, src_dt):
    T, N, F, W = geom
    rng = np.random.default_rng([T, N, F, W, src_dt])
    ndt = np.float32 if src_dt == F32 else np.float16

    def nonzero(shape):
        v = rng.standard_normal(shape)
        return (np.sign(v) * (0.5 + np.abs(v))).astype(ndt)

    frames, init = nonzero((T, N, W)), nonzero((N, F * W))
    init[:, -W:] = frames[0]  # the stack at step 0 ends with step 0's frame
    dones = _stack_dones(rng, T, N, F)
    ref = RR.stack_replay(init, frames, dones, F, W)
    kinds = _stack_kinds(ref, dones, T, N, F, W)
    assert _stack_required(T, N, F, W) <= kinds, (geom, sorted(kinds))
    for a in (frames, init, dones, ref):
        a.setflags(write=False)
    return frames, init, dones, ref


def test_stack_cases_show_every_planted_kind():
    """The reference alone (no device): every geometry with F > 1 and T > 1 has rows of each planted
    kind that the geometry admits."""
    for geom in GEOMS:
        for src_dt in (F32, F16):
            _stack_case(geom, src_dt)
    assert _stack_required(30, 8, 15, 47) == {"a", "b", "c", "d", "d2", "e", "f"}
    assert _stack_required(4, 3, 6, 5) == {"a", "d", "d2", "e", "f"}  # T < F: tau < 0 on every row


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{TDT[p[0]]}-{TDT[p[1]]}".replace("torch.", ""))
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=lambda i: "x".join(map(str, GEOMS[i])))
def test_gather_stacked(gi, pair):
    """hg_gather_stacked == the deque stepped literally (rollout_ref.stack_replay), cast by torch on
    the CPU, bitwise, for every dtype pair, both dones layouts, an identity index and a shuffled one
    with duplicates whose length is no multiple of 4, with plain tables of the early and late
    paths gathered by the same launch."""
    _need_gpu()
    from humanoid import _native as N_
    L = _lib()
    geom = GEOMS[gi]
    T, N, F, W = geom
    sd, dd = pair
    frames, init, dones, ref = _stack_case(geom, sd)
    want_all = torch.from_numpy(np.array(ref.reshape(T * N, F * W))).to(TDT[dd])
    frames_d = _dev(frames.transpose(1, 0, 2))  # env-major [N, T, W]
    init_d = _dev(init)
    lay = {"time": (_dev(dones), N, 1), "env": (_dev(dones.T), 1, T)}
    rng = np.random.default_rng([gi, sd, dd])
    total = T * N
    ln = total + 1 if (total + 1) % 4 else total + 2
    for li, (layout, ident) in enumerate(itertools.product(("time", "env"), (True, False))):
        idx = np.arange(total) if ident else rng.integers(0, total, ln)
        rows = len(idx)
        assert ident or rows % 4 != 0
        idx_d = _dev(idx.astype(np.int64))
        spec = PLAIN[(gi * 4 + li) % len(PLAIN)]
        src = [_table(rng, total, s[0], s[1], s[3]) for s in spec]
        src_d = [t.to(DEV) for t in src]
        pdst = [Guarded(rows, s[0], TDT[s[2]]) for s in spec]
        tabs = (N_.GatherTable * max(len(spec), 1))(*[N_.GatherTable(t.data_ptr(), g.ptr, s[0], s[1], s[2])
                                                      for s, t, g in zip(spec, src_d, pdst)])
        dst = Guarded(rows, F * W, TDT[dd])
        dn, dts, des = lay[layout]
        rc = L.hg_gather_stacked(idx_d.data_ptr(), rows, frames_d.data_ptr(), init_d.data_ptr(), dn.data_ptr(), dts,
                                 des, T, N, F, W, sd, dst.ptr, dd, tabs if spec else None, len(spec), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        it = torch.from_numpy(idx)
        got = dst.get()
        if not _same_bits(got, want_all[it]):
            bad = (_bits(got) != _bits(want_all[it])).any(1).nonzero()[:, 0].tolist()
            raise AssertionError(f"{geom} {layout} ident={ident}: rows {bad[:8]} (storage rows {idx[bad[:8]]}) differ")
        for s, t, g in zip(spec, src, pdst):
            assert _same_bits(g.get(), t[it].to(TDT[s[2]])), (geom, s)


def test_gather_stacked_rejections():
    _need_gpu()
    from humanoid import _native as N_
    L = _lib()
    T, N, F, W = 3, 2, 2, 4
    frames, init = torch.ones(N, T, W, device=DEV), torch.ones(N, F * W, device=DEV)
    dones = torch.zeros(T, N, dtype=torch.uint8, device=DEV)
    idx = torch.arange(T * N, device=DEV)
    dst, p = Guarded(T * N, 64 * W + W), Guarded(T * N, 4)
    src = torch.ones(T * N, 4, device=DEV)
    tabs = (N_.GatherTable * 3)(*[N_.GatherTable(src.data_ptr(), p.ptr, 4, F32, F32)] * 3)

    def call(F_=F, ntab=0, sd=F32, dd=F32):
        return L.hg_gather_stacked(idx.data_ptr(), T * N, frames.data_ptr(), init.data_ptr(), dones.data_ptr(), N, 1,
                                   T, N, F_, W, sd, dst.ptr, dd, tabs, ntab, _stream())

    assert call(F_=0) == HG_ERR_ARG and call(F_=65) == HG_ERR_ARG and call(ntab=3) == HG_ERR_ARG
    assert call(sd=BF16, dd=BF16) == HG_ERR_ARG and call(sd=BF16, dd=F32) == HG_ERR_ARG
    assert call(sd=F32, dd=F16) == HG_ERR_ARG
    torch.cuda.synchronize()
    assert dst.untouched() and p.untouched()
