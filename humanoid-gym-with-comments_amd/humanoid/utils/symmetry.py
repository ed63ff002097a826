"""Left/right mirror tables of XBot-L for PPO's symmetry loss (humanoid/algo/ppo/ppo.py:59-63,
93-105, 197-208 of the reference: ``sym_loss``, ``obs_permutation``, ``act_permutation``).

The reference's format is a list of signed source indices: entry ``c`` of a table says that column
``c`` of the mirrored vector is column ``abs(p)`` of the original, negated when ``p < 0``.  Column 0
cannot carry a sign that way, so it is written as a small negative number (``-0.0001``) when it is
negated — ``int(abs(-0.0001)) == 0`` — the usual idiom of such tables.

XBot-L's twelve leg joints are ordered left leg (roll, yaw, pitch, knee, ankle pitch, ankle roll)
then right leg, and the URDF's right-leg axes are laid out so that the mirrored pose is "swap the
legs and negate all twelve joints" (the right-leg limits are the negated left-leg limits;
tests/test_symmetry_tables.py checks the map against the oracle's forward kinematics).  Reflecting
the world in the x-z plane maps a vector (x, y, z) to (x, -y, z) and a pseudo-vector (angular
velocity, Euler angles) to (-x, y, -z).
"""
import numpy as np

NUM_DOF = 12
FRAME = 47  # [sin, cos, cmd_x, cmd_y, cmd_yaw, q 12, qd 12, a 12, omega 3, euler 3]

# the joint map as (perm, sign): mirrored[j] = sign[j] * original[perm[j]]
JOINT_PERM = np.array([(j + 6) % NUM_DOF for j in range(NUM_DOF)], dtype=np.int64)
JOINT_SIGN = -np.ones(NUM_DOF, dtype=np.float64)


def _signed(index, negative):
    """One entry of a reference-format table."""
    if not negative:
        return float(index)
    return -float(index) if index else -0.0001


def xbotl_mirror():
    """(obs_permutation [47], act_permutation [12]) in the reference's signed-index format for one
    actor observation frame (humanoid_env.py compute_observations: sin, cos, the three commands,
    q - default, qd, the last action, the base angular velocity and the base Euler angles):
    the gait phase shifts by half a cycle (sin and cos negated: the legs swap roles), cmd_x kept,
    cmd_y and cmd_yaw negated, each 12-block through the joint map, omega and the Euler angles
    (-, +, -)."""
    obs = [_signed(0, True), _signed(1, True), _signed(2, False), _signed(3, True), _signed(4, True)]
    for base in (5, 17, 29):
        obs += [_signed(base + int(JOINT_PERM[j]), JOINT_SIGN[j] < 0) for j in range(NUM_DOF)]
    for base in (41, 44):
        obs += [_signed(base, True), _signed(base + 1, False), _signed(base + 2, True)]
    act = [_signed(int(JOINT_PERM[j]), JOINT_SIGN[j] < 0) for j in range(NUM_DOF)]
    assert len(obs) == FRAME
    return obs, act


def table_arrays(permutation):
    """(perm int64, sign float32) of a reference-format table: source column ``int(abs(p))``,
    negative iff ``p < 0``."""
    perm = np.array([int(abs(p)) for p in permutation], dtype=np.int64)
    sign = np.array([-1.0 if p < 0 else 1.0 for p in permutation], dtype=np.float32)
    return perm, sign


def stack_table(permutation, frame_stack):
    """The table of ``frame_stack`` stacked frames, as ppo.py:99-102 builds it: frame ``i``'s
    entries offset by ``i * len(permutation)``, signs kept."""
    n = len(permutation)
    return [(-1.0 if p < 0 else 1.0) * (abs(p) + i * n) for i in range(frame_stack) for p in permutation]


def mirror_state(root, q, qd):
    """The mirrored simulator state: root [.., 13] (position, quaternion xyzw, linear velocity,
    angular velocity), q / qd [.., 12].  Position (x, -y, z), quaternion (-x, y, -z, w), linear
    velocity (+, -, +), angular velocity (-, +, -); joints through the joint map."""
    root = np.asarray(root)
    s = np.array([1, -1, 1, -1, 1, -1, 1, 1, -1, 1, -1, 1, -1], dtype=root.dtype)
    q, qd = np.asarray(q), np.asarray(qd)
    js = JOINT_SIGN.astype(q.dtype)
    return root * s, q[..., JOINT_PERM] * js, qd[..., JOINT_PERM] * js
