"""XBot-L's mirror tables for PPO's symmetry loss (humanoid/utils/symmetry.py) and the argument
checks of the symmetry kernels' C entries (CPU only: every call here is refused before a launch).

The joint map "swap the legs, negate all twelve joints" is checked against the oracle's forward
kinematics (oracle/physics_ref.rigid_states): at the mirrored pose the right foot's four sole
corners, reflected in the x-z plane, are the left foot's.  Measured with the shipped map: 1.2e-5 m
over 256 in-limit poses (the model's own left/right asymmetry at q = 0 is 5e-6 m); the bound is
1e-4 m, 8x that and 100x below the smallest single-sign mutant (0.06 m, the ankle roll).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from humanoid import _native as N
from humanoid.utils import symmetry as S


def _apply(table, x):
    perm, sign = S.table_arrays(table)
    return x[..., perm] * sign


def test_tables_are_signed_involutions():
    obs, act = S.xbotl_mirror()
    assert len(obs) == S.FRAME == 47 and len(act) == 12
    for table in (obs, act):
        assert all(p != 0 for p in table), "a literal 0 entry carries no sign"
        perm, sign = S.table_arrays(table)
        assert sorted(perm.tolist()) == list(range(len(table)))
        assert set(np.abs(sign).tolist()) == {1.0}
        x = np.random.default_rng(1).standard_normal((3, len(table)))
        np.testing.assert_array_equal(_apply(table, _apply(table, x)), x)
    # the table's rows, spelled out
    perm, sign = S.table_arrays(obs)
    assert perm[:5].tolist() == [0, 1, 2, 3, 4] and sign[:5].tolist() == [-1, -1, 1, -1, -1]
    for base in (5, 17, 29):
        assert perm[base:base + 12].tolist() == [base + (j + 6) % 12 for j in range(12)]
        assert (sign[base:base + 12] == -1).all()
    assert perm[41:].tolist() == list(range(41, 47)) and sign[41:].tolist() == [-1, 1, -1, -1, 1, -1]
    ap, asg = S.table_arrays(act)
    assert ap.tolist() == S.JOINT_PERM.tolist() and (asg == S.JOINT_SIGN).all()


def test_stacked_table_repeats_the_frame():
    obs, _ = S.xbotl_mirror()
    perm, sign = S.table_arrays(S.stack_table(obs, 15))
    p1, s1 = S.table_arrays(obs)
    assert perm.shape == (705,)
    np.testing.assert_array_equal(perm, np.concatenate([p1 + 47 * i for i in range(15)]))
    np.testing.assert_array_equal(sign, np.tile(s1, 15))


def test_ppo_matrices_equal_the_signed_gather():
    """PPO(sym_loss=True) on the CPU: x @ obs_perm_mat / a @ act_perm_mat (the reference's
    products, ppo.py:199-201) are the signed gathers of the tables."""
    from humanoid.algo.ppo import ActorCritic, PPO
    obs, act = S.xbotl_mirror()
    ac = ActorCritic(705, 219, 12, actor_hidden_dims=[8], critic_hidden_dims=[8], base_lin_vel_hidden_dims=[8])
    ppo = PPO(ac, device="cpu", sym_loss=True, obs_permutation=obs, act_permutation=act, frame_stack=15)
    assert ppo._sym_tables is None and not ppo._fused_loss  # the CPU keeps the op-by-op expression
    x = torch.randn(5, 705, dtype=torch.float64)
    want = _apply(S.stack_table(obs, 15), x.numpy())
    np.testing.assert_array_equal((x @ ppo.obs_perm_mat.double()).numpy(), want)
    a = torch.randn(5, 12, dtype=torch.float64)
    np.testing.assert_array_equal((a @ ppo.act_perm_mat.double()).numpy(), _apply(act, a.numpy()))
    for mat in (ppo.obs_perm_mat, ppo.act_perm_mat):
        np.testing.assert_array_equal((mat @ mat).numpy(), np.eye(mat.shape[0], dtype=np.float32))


def test_mirror_state_is_an_involution():
    rng = np.random.default_rng(2)
    root, q, qd = rng.standard_normal((4, 13)), rng.standard_normal((4, 12)), rng.standard_normal((4, 12))
    r2, q2, qd2 = S.mirror_state(*S.mirror_state(root, q, qd))
    for got, want in ((r2, root), (q2, q), (qd2, qd)):
        np.testing.assert_array_equal(got, want)
    r1, _, _ = S.mirror_state(root, q, qd)
    np.testing.assert_array_equal(r1[:, [1, 3, 5, 8, 10, 12]], -root[:, [1, 3, 5, 8, 10, 12]])
    np.testing.assert_array_equal(r1[:, [0, 2, 4, 6, 7, 9, 11]], root[:, [0, 2, 4, 6, 7, 9, 11]])


def _sole_deviation(perm, sign):
    """Per pose, the distance between the left foot's sole corners at q and the y-reflected right
    foot's at the mirrored pose (as point sets), base at the origin, upright."""
    import physics_ref as P
    m, js = N.load_model()
    limits = np.array(N.model_names(js)[3])
    lo, hi = limits[:, 0], limits[:, 1]
    q = np.random.default_rng(0).uniform(lo, hi, size=(256, 12))
    qm = q[:, perm] * sign
    root = np.zeros((256, 13))
    root[:, 6] = 1.0
    refl = np.array([1.0, -1.0, 1.0])
    body = np.array([m.contact_body[c] for c in range(m.num_contacts)])
    left = P.ground_candidates(m, P.rigid_states(m, root, q, 0 * q))[:, body == 6]
    right = (P.ground_candidates(m, P.rigid_states(m, root, qm, 0 * q)) * refl)[:, body == 12]
    assert left.shape[1] == right.shape[1] == 4
    d = np.linalg.norm(left[:, :, None] - right[:, None], axis=-1)
    inside = bool((qm >= lo - 1e-12).all() and (qm <= hi + 1e-12).all())
    return np.maximum(d.min(2).max(1), d.min(1).max(1)), inside


def test_joint_map_against_oracle_forward_kinematics():
    dev, inside = _sole_deviation(S.JOINT_PERM, S.JOINT_SIGN)
    print("shipped map: max sole-corner deviation", dev.max())
    assert inside, "the mirrored poses leave the joint limits"
    assert dev.max() <= 1e-4
    for k in range(6):  # one joint's sign flipped (on both legs: still an involution)
        sign = S.JOINT_SIGN.copy()
        sign[[k, k + 6]] *= -1
        worst = _sole_deviation(S.JOINT_PERM, sign)[0].max()
        print("mutant", k, "max deviation", worst)
        assert worst > 1e-2, f"flipping joint {k}'s sign went undetected ({worst} m)"


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(N.LIB_PATH):
        pytest.skip("libhgsim.so not built")
    return N.load_library()


FAKE, FAKE2 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)  # never dereferenced on a refused call


def test_mirror_rows_rejects_bad_arguments(L):
    args = dict(src=FAKE, src_ld=705, dst=FAKE2, dst_ld=705, rows=24, width=705, perm=FAKE, sign=FAKE)

    def call(**kw):
        a = dict(args, **kw)
        return L.hg_mirror_rows(a["src"], a["src_ld"], a["dst"], a["dst_ld"], a["rows"], a["width"], a["perm"],
                                a["sign"], None)
    for bad in (dict(src=None), dict(dst=None), dict(perm=None), dict(sign=None), dict(rows=0), dict(rows=-3),
                dict(width=0), dict(src_ld=704), dict(dst_ld=704), dict(dst=FAKE)):
        assert call(**bad) == 1, bad  # HG_ERR_ARG


def test_sym_loss_rejects_bad_arguments(L):
    names = ("mu", "mu_ld", "mir", "mir_ld", "perm", "sign", "rows", "A", "coef", "loss", "sym", "g_mu", "g_mir",
             "scratch")
    args = dict(mu=FAKE, mu_ld=12, mir=FAKE2, mir_ld=12, perm=FAKE, sign=FAKE, rows=24, A=12, coef=1.0, loss=FAKE,
                sym=FAKE, g_mu=FAKE, g_mir=FAKE2, scratch=FAKE)

    def call(**kw):
        a = dict(args, **kw)
        return L.hg_sym_loss(*[a[n] for n in names], None)
    bad = [{n: None} for n in ("mu", "mir", "perm", "sign", "loss", "sym", "g_mu", "g_mir", "scratch")]
    bad += [dict(rows=0), dict(A=0), dict(A=N.HG_MAX_DOF + 1, mu_ld=64, mir_ld=64), dict(mu_ld=11), dict(mir_ld=11)]
    for b in bad:
        assert call(**b) == 1, b
    assert L.hg_sym_loss_scratch(24576, 12) == 384 and L.hg_sym_loss_scratch(1, 12) == 1


def test_sym_loss_backward_rejects_bad_arguments(L):
    def call(g=FAKE, rows=24, A=12, g_mu=FAKE, g_mir=FAKE2):
        return L.hg_sym_loss_backward(g, rows, A, g_mu, g_mir, None)
    for bad in (dict(g=None), dict(g_mu=None), dict(g_mir=None), dict(rows=0), dict(A=0)):
        assert call(**bad) == 1, bad
