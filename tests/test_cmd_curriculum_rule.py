"""The command curriculum's rule (reference update_command_curriculum + the order of reset_idx,
humanoid_env.py:1097-1106, 1120-1129, 1148-1149) restated in numpy and pinned against the
reference's own results (tests/golden/cmd_curriculum.npz, tests/golden/gen_cmd_curriculum.py);
the GPU tests take their expected ranges from ``curriculum_rule``.  Plus the C ABI of the feature:
the new export, the two hg_cfg fields, the new tensor ids."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from humanoid import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "hgsim.h")
GOLDEN = os.path.join(REPO, "tests", "golden", "cmd_curriculum.npz")


def curriculum_rule(sums, ids, counter, rng, max_curriculum, max_episode_length, reward_scale):
    """command_ranges["lin_vel_x"] after reset_idx(ids) at common_step_counter `counter`, in
    float64: sums [N] are the tracking_lin_vel episode sums, reward_scale carries dt."""
    lo, hi = float(rng[0]), float(rng[1])
    ids = np.asarray(ids)
    if len(ids) and counter % int(max_episode_length) == 0:
        mean = np.mean(np.asarray(sums)[ids].astype(np.float64))
        if mean / max_episode_length > 0.8 * reward_scale:
            lo = float(np.clip(lo - 0.5, -max_curriculum, 0.0))
            hi = float(np.clip(hi + 0.5, 0.0, max_curriculum))
    return lo, hi


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _rule_on(golden, tag):
    g = lambda k: golden[f"{tag}/{k}"]  # noqa: E731
    return curriculum_rule(g("sums"), g("ids"), int(g("counter")), g("range_in"), float(g("max_curriculum")),
                           float(g("max_episode_length")), float(g("reward_scale")))


def test_rule_matches_the_reference(golden):
    cases = [str(c) for c in golden["cases"]]
    assert cases == ["above", "below", "chain0", "chain1", "chain2", "offstep", "initial"]
    for tag in cases:
        want = golden[f"{tag}/range_out"]
        assert _rule_on(golden, tag) == (want[0], want[1]), tag
        # extras["episode"]["max_command_x"] is the upper bound after the update
        assert float(golden[f"{tag}/max_command_x"]) == want[1], tag


def test_golden_covers_the_stated_cases(golden):
    thr = 0.8 * 1.2 * 0.01 * 2400
    assert abs(float(golden["above/reward_scale"]) * 0.8 * float(golden["above/max_episode_length"]) - thr) < 1e-9
    mean = lambda tag: golden[f"{tag}/sums"][golden[f"{tag}/ids"]].astype(np.float64).mean()  # noqa: E731
    assert abs(mean("above") / thr - 1.02) < 1e-3 and abs(mean("below") / thr - 0.98) < 1e-3
    np.testing.assert_array_equal(golden["above/range_out"], [-0.8, 1.1])
    np.testing.assert_array_equal(golden["below/range_out"], [-0.3, 0.6])
    np.testing.assert_array_equal(golden["chain0/range_in"], [-0.3, 0.6])
    np.testing.assert_array_equal(golden["chain0/range_out"], [-0.8, 1.0])
    np.testing.assert_array_equal(golden["chain1/range_out"], [-1.0, 1.0])
    np.testing.assert_array_equal(golden["chain2/range_out"], [-1.0, 1.0])
    assert int(golden["offstep/counter"]) % 2400 != 0 and mean("offstep") > thr
    np.testing.assert_array_equal(golden["offstep/range_out"], [-0.3, 0.6])
    assert int(golden["initial/counter"]) == 0 and len(golden["initial/ids"]) == len(golden["initial/sums"])
    np.testing.assert_array_equal(golden["initial/range_out"], [-0.3, 0.6])
    # the other envs' sums would flip the decision if they were averaged in
    for tag in ("above", "below"):
        s = golden[f"{tag}/sums"]
        assert (s.astype(np.float64).mean() > thr) != (mean(tag) > thr), tag


def test_reset_commands_are_drawn_from_the_updated_range(golden):
    """reset_idx updates the range before _resample_commands (:1120-1129): the recorded commands
    are torch_rand_float(lo', hi', u) of the recorded uniforms with the range coming OUT."""
    f32 = np.float32
    for tag in [str(c) for c in golden["cases"]]:
        u = golden[f"{tag}/cmd_u"].astype(f32)
        lo, hi = golden[f"{tag}/range_out"]
        ylo, yhi = golden[f"{tag}/range_y"]
        cx = (f32(hi - lo) * u[:, 0] + f32(lo)).astype(f32)
        cy = (f32(yhi - ylo) * u[:, 1] + f32(ylo)).astype(f32)
        keep = (np.sqrt(cx * cx + cy * cy) > 0.2).astype(f32)
        cmd = golden[f"{tag}/commands"]
        np.testing.assert_allclose(cmd[:, 0], cx * keep, rtol=0, atol=1e-6, err_msg=tag)
        np.testing.assert_allclose(cmd[:, 1], cy * keep, rtol=0, atol=1e-6, err_msg=tag)
    # and where the range moved, the old range gives other commands
    u = golden["above/cmd_u"].astype(f32)
    lo, hi = golden["above/range_in"]
    old = (f32(hi - lo) * u[:, 0] + f32(lo)).astype(f32)
    assert np.abs(old - golden["above/commands"][:, 0]).max() > 0.05


# ---------------------------------------------------------------------------------------- C ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_new_exports_are_in_the_header():
    src = _header()
    for name in ("hg_set_command_range_x", "hg_publish_terrain_level"):
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in N.EXPORTS
    if os.path.exists(N.LIB_PATH):
        L = N.load_library()
        assert L.hg_set_command_range_x(None, -0.3, 0.6, None) != 0  # null handle: refused, nothing launched
        assert L.hg_publish_terrain_level(None, 1) != 0


def test_tensor_ids_match_the_header():
    body = re.search(r"enum hg_tensor_id \{(.*?)HG_T_COUNT", _header(), flags=re.S).group(1)
    ids = re.findall(r"HG_T_([A-Z_]+)", body)
    assert ids == N.TENSOR_IDS
    assert ids[-2:] == ["CMD_RANGE_X", "CURRICULUM_RING"]  # appended: every earlier id keeps its value


def test_cfg_fields_sit_after_terrain_origins(tmp_path):
    names = [f[0] for f in N.HgCfg._fields_]
    assert names[-3:] == ["terrain_origins", "cmd_curriculum", "cmd_max_curriculum"]
    end = N.HgCfg.terrain_origins.offset + ctypes.sizeof(ctypes.c_void_p)
    assert N.HgCfg.cmd_curriculum.offset == end and N.HgCfg.cmd_max_curriculum.offset == end + 4
    c = tmp_path / "off.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hgsim.h"\nint main(){printf("%zu %zu %zu %zu",'
                 'offsetof(hg_cfg,terrain_origins),offsetof(hg_cfg,cmd_curriculum),'
                 'offsetof(hg_cfg,cmd_max_curriculum),sizeof(hg_cfg));}')
    exe = tmp_path / "off"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [N.HgCfg.terrain_origins.offset, N.HgCfg.cmd_curriculum.offset,
                   N.HgCfg.cmd_max_curriculum.offset, ctypes.sizeof(N.HgCfg)]


def test_build_hg_cfg_fills_the_curriculum_fields():
    from humanoid.envs import XBotLCfg
    from humanoid.envs.custom.humanoid_env import build_hg_cfg
    _, js = N.load_model()
    cfg = XBotLCfg()
    c, _ = build_hg_cfg(cfg, 8, 0.001, 5, js)
    assert c.cmd_curriculum == 0 and c.cmd_max_curriculum == np.float32(cfg.commands.max_curriculum)
    cfg.commands.curriculum = True
    cfg.commands.max_curriculum = 1.5
    c, _ = build_hg_cfg(cfg, 8, 0.001, 5, js)
    assert c.cmd_curriculum == 1 and c.cmd_max_curriculum == 1.5
    assert (c.cmd_lin_x[0], c.cmd_lin_x[1]) == (np.float32(-0.3), np.float32(0.6))
