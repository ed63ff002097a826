"""k_post_step (csrc/hg_envlogic.hip) on the planted rows of oracle/post_cases.py: one env per row,
every branch of the 22 reward terms, the termination, the heading command and the ~30 observation
clips taken on both sides at a stated margin (tests/test_post_cases.py holds the table to that on
the CPU), one hg_post for the whole table.

  flags and discrete state   reset_buf, time_out_buf, episode_length_buf, last_contacts and the
                             stance / contact-mask columns of the privileged frame: exact
  per-term episode sums      planted 0 on the rows that stay, so _sums[k] is the term x its scale:
                             against the float64 term within the derived float32 bound of
                             post_cases.term_bounds; the five terms that replay exact selections
                             (collision, feet_air_time, feet_clearance, feet_contact_number,
                             low_speed) bitwise against the float32 oracle
  resetting rows             _sums cleared; the episode statistics through _check_episode_stats
  total reward               against max(sum of the float64 increments, 0) within the total's bound;
                             the clearly negative rows exactly 0
  carried state              feet_air_time, feet_height, last_feet_z bitwise; commands, ref_dof_pos
  observation frames         planted clip entries exactly +-clip_observations in both tables, their
                             partners just inside not clipped, everything else at _post_parity's
                             tolerance; with add_noise on and off

What would fail if the kernel were wrong is recorded in DESIGN.md section 2 (mutation record)."""
import numpy as np
import pytest
import torch

import post_cases as PC
from test_gpu_parity import _check_episode_stats, _make_env, _need_gpu, _oracle_cfg, _post_once, snapshot

pytestmark = pytest.mark.gpu

FIELDS = ("root_states", "dof_pos", "dof_vel", "contact_forces", "rigid_state", "torques", "actions", "last_actions",
          "last_last_actions", "last_dof_vel", "last_root_vel", "commands", "feet_air_time", "last_contacts", "feet_height",
          "last_feet_z", "env_frictions", "body_mass", "rand_push_force", "rand_push_torque", "ref_dof_pos")


def _run(add_noise):
    """One env of PC.N rows with the planted table written through its views, one hg_post, and the
    oracle on the snapshot of what the env held."""
    env = _make_env(PC.N, noise__add_noise=add_noise)
    assert bool(env._hgcfg.add_noise) == add_noise
    cfg = _oracle_cfg(env)
    S0, _, _ = snapshot(env)
    A, tb = PC.plant(S0, cfg)
    dev = env.root_states.device
    for k in FIELDS:
        getattr(env, k).copy_(torch.from_numpy(np.ascontiguousarray(A[k])).to(dev))
    env.episode_length_buf.copy_(torch.from_numpy(A["episode_length_buf"]).to(dev))
    env._sums.copy_(torch.from_numpy(np.stack([A["episode_sums"][nm] for nm in PC.NAMES])).to(dev))
    S, hist_o, hist_p = snapshot(env)
    for k in FIELDS + ("episode_length_buf",):   # the views took the table as it is
        np.testing.assert_array_equal(S[k], A[k], err_msg=k)
    ref = PC.reference(S, hist_o, hist_p, cfg, PC.COUNTER)
    _post_once(env, PC.COUNTER)
    env._publish_extras()
    after, obs, priv = snapshot(env)
    g = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    got = PC.collect(after, obs, priv, g(env.rew_buf), g(env.reset_buf), g(env.time_out_buf))
    return env, cfg, tb, ref, got


@pytest.fixture(scope="module", params=[True, False], ids=["noise", "no_noise"])
def run(request):
    _need_gpu()
    return _run(request.param)


def test_planted_rows(run):
    env, cfg, tb, ref, got = run
    bad, worst = PC.check(got, ref, tb, cfg)
    print("k_post_step |gpu - f64| / bound:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert bad == [], "\n".join(bad)


def test_episode_statistics_of_the_resetting_rows(run):
    env, cfg, tb, ref, got = run
    rid = np.nonzero(ref["reset"])[0]
    assert len(rid) >= 10
    after = {nm: (ref["planted_sums"][nm] + ref["inc32"][nm]).astype(np.float32) for nm in PC.NAMES}
    np.testing.assert_array_equal(got["timeout"], env.extras["time_outs"].cpu().numpy())
    _check_episode_stats(env, after, rid, ref["extras"]["episode"], label=f"planted rows n={PC.N}")
