"""Self-checks of oracle/rollout_ref.py, the numpy references tests/test_gpu_rollout_abi.py holds the
rollout kernels to.  No GPU: the references are checked against oracle/rng_ref.py, against each
other, and against hand-written cases; and the inputs the GPU tests use are shown to discriminate
(a dropped row offset, a lost counter high word or a lost seed high word changes the draws)."""
import numpy as np

import rng_ref as R
import rollout_ref as RR

SEEDS = (0x9E3779B97F4A7C15, 0x0123456700000005)
BIG = (1 << 32) + 5


def test_purpose_constant():
    assert RR.ACTION_SAMPLE == 9 and RR.ACTION_SAMPLE not in (
        R.ACT_DELAY, R.ACT_NOISE, R.OBS_NOISE, R.CMD, R.PUSH, R.RESET_DOF, R.RESET_ROOT, R.TERRAIN)


def test_float32_draws_are_rng_ref_normals():
    for seed, off, ctr, n, A in ((SEEDS[0], 0, 0, 33, 12), (SEEDS[1], 4096, BIG, 17, 64), (5, 3, 7, 5, 1),
                                 (SEEDS[0], 4096, 7, 9, 17)):
        want = R.normals(seed, np.arange(n) + off, ctr, purpose=9, count=A)
        got = RR.act_normals(seed, off, ctr, n, A)
        assert got.dtype == np.float32 and got.shape == (n, A)
        np.testing.assert_array_equal(got, want)


def test_float64_draws_bound_the_float32_oracle():
    """|z32 - z64| <= 2 * 2^-23 * r per draw (measured: 1.55 in these units over the 160k draws of
    the two seeds below, one of them at a counter above 2^32)."""
    worst = 0.0
    for seed, ctr in ((SEEDS[0], 7), (SEEDS[1], BIG)):
        z32 = RR.act_normals(seed, 4096, ctr, 5000, 16)
        z64, r = RR.act_normals64(seed, 4096, ctr, 5000, 16)
        assert z64.dtype == np.float64 and r.shape == z64.shape == (5000, 16)
        # the radius belongs to the draw: z0^2 + z1^2 = r^2 for each Box-Muller pair
        np.testing.assert_allclose(z64[:, 0::2] ** 2 + z64[:, 1::2] ** 2, r[:, 0::2] ** 2, rtol=1e-12, atol=1e-300)
        np.testing.assert_array_equal(r[:, 0::2], r[:, 1::2])
        units = np.abs(z32.astype(np.float64) - z64) / (2.0 ** -23 * r)
        worst = max(worst, float(units.max()))
        z = z64.ravel()
        assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    print(f"float32 oracle vs float64: {worst:.3f} x 2^-23 r")
    assert worst <= 2.0


def test_inputs_discriminate():
    """The GPU test inputs must tell the bugs apart: the draws change with the row offset, with the
    counter's high word and with the seed's high word, and each Box-Muller lane is distinct."""
    n, A = 64, 12
    base = RR.act_normals(SEEDS[0], 0, 5, n, A)
    assert not np.array_equal(base, RR.act_normals(SEEDS[0], 4096, 5, n, A))
    assert not np.array_equal(base, RR.act_normals(SEEDS[0], 0, BIG, n, A))
    assert not np.array_equal(base, RR.act_normals(SEEDS[0] ^ (1 << 40), 0, 5, n, A))
    # row offset 4096 is env 4096 + e of the unshifted stream, not a reshuffle of the same rows
    np.testing.assert_array_equal(RR.act_normals(SEEDS[0], 4096, 5, n, A),
                                  RR.act_normals(SEEDS[0], 0, 5, 4096 + n, A)[4096:])
    # every row differs in every element, far beyond the GPU test's bound (4 * 2^-23 r)
    z64, r = RR.act_normals64(SEEDS[0], 0, 5, n, A)
    for other in (RR.act_normals64(SEEDS[0], 4096, 5, n, A)[0], RR.act_normals64(SEEDS[0], 0, BIG, n, A)[0],
                  RR.act_normals64(SEEDS[0] ^ (1 << 40), 0, 5, n, A)[0]):
        assert (np.abs(other - z64) > 4 * 2.0 ** -23 * r).mean() > 0.99
    # a wrong lane (j & 3) or a wrong block (j >> 2) is another number
    for j in range(A):
        for k in range(A):
            if j != k:
                assert (np.abs(z64[:, j] - z64[:, k]) > 4 * 2.0 ** -23 * r[:, j]).mean() > 0.95


def test_log_prob64_and_bootstrap64():
    a = np.array([[0.5, -1.0], [0.0, 0.0]])
    mu = np.array([[0.0, 1.0], [0.0, 0.0]])
    sg = np.array([1.0, 2.0])
    lp, S = RR.log_prob64(a, mu, sg)
    c = 0.5 * np.log(2 * np.pi)
    np.testing.assert_allclose(lp, [-0.125 - 0.5 - np.log(2.0) - 2 * c, -np.log(2.0) - 2 * c], rtol=1e-15)
    np.testing.assert_allclose(S, [0.125 + 0.5 + np.log(2.0) + 2 * c, np.log(2.0) + 2 * c], rtol=1e-15)
    # a dropped log sigma term is far above the GPU test's bound (A + 8) 2^-24 S at sigma = 0.99
    lp1, S1 = RR.log_prob64(np.zeros((1, 12)), np.zeros((1, 12)), np.full(12, 0.99))
    assert abs(12 * np.log(0.99)) > 1e3 * 20 * 2.0 ** -24 * S1[0]
    out = RR.bootstrap64([1.0, 2.0], [10.0, 10.0], [0, 1], 0.994)
    np.testing.assert_array_equal(out, [1.0, 2.0 + float(np.float32(0.994)) * 10.0])


def test_stack_replay_is_the_shifted_previous_stack():
    """The identity test_obs_window_stacking_over_wraps asserts of the env's windows:
    stack[t + 1][:, :(F - 1) W] == 0 if reset else stack[t][:, W:], the newest frame last."""
    rng = np.random.default_rng(3)
    T, N, F, W = 12, 5, 4, 3
    frames = rng.standard_normal((T, N, W)).astype(np.float32)
    init = rng.standard_normal((N, F * W)).astype(np.float32)
    init[:, -W:] = frames[0]
    dones = (rng.random((T, N)) < 0.3).astype(np.uint8)
    st = RR.stack_replay(init, frames, dones, F, W)
    assert st.shape == (T, N, F * W) and st.dtype == np.float32
    np.testing.assert_array_equal(st[0], init)
    for t in range(T - 1):
        rs = dones[t].astype(bool)[:, None]
        np.testing.assert_array_equal(st[t + 1][:, :-W], np.where(rs, 0, st[t][:, W:]))
        np.testing.assert_array_equal(st[t + 1][:, -W:], frames[t + 1])
    assert dones[:-1].any() and not dones[:-1].all()


def test_stack_replay_literal():
    F, W = 3, 2
    init = np.array([[1, 2, 3, 4, 5, 6]], np.float32)
    frames = np.array([[[5, 6]], [[7, 8]], [[9, 10]], [[11, 12]]], np.float32)
    dones = np.array([[0], [1], [0], [1]], np.uint8)  # the last one is after the last row
    st = RR.stack_replay(init, frames, dones, F, W)
    want = np.array([[[1, 2, 3, 4, 5, 6]],
                     [[3, 4, 5, 6, 7, 8]],
                     [[0, 0, 0, 0, 9, 10]],      # the reset of step 1 cleared the history
                     [[0, 0, 9, 10, 11, 12]]], np.float32)
    np.testing.assert_array_equal(st, want)
