"""The light part of the regular substep -- the flag masks read once at its top, the joint motors as one lane phase, the
"arm far" and "arm static" decisions, wake stage 1 and 2, the island closure of the body-velocity phase and the closing
tests (rv_dev_env.h: sim_substep_light, arm_motor_lanes) -- on both builds of the env kernel against the float oracle,
bit for bit: body states, joint states, env counters, manifold counts and link poses (no tolerance anywhere in this
file).

One scene per path of that code, 32 envs each; a scripted scene differs from env to env (offsets and yaw by the env's
index).  Each case first asserts ON THE ORACLE'S DATA that the scene is what it claims, so a scene that stops reaching
its case fails -- without a GPU -- and does not pass empty; the oracle's side of a case is computed once per module
and is read-only afterwards.

  (a) the arm wakes a sleeper                      -> two boxes asleep in a row, the gripper driven at them: launches in
                                                      which stage 1 says no, then flags with a bound left, then queries, then
                                                      the hit
  (b) the closure and the moving-neighbour wake    -> case (a)'s second box: woken through a pair manifold that holds points
                                                      in some envs, by the moving first box in the others
  (c) "arm far" with a body awake                  -> a box thrown along the far side of the table while the arm follows a
                                                      joint target well away from everything
  (d) arm static                                   -> a box dropped beside the resting arm: no joint changes, a body awake
  (e) the quiet substep; at_possible, nobody awake -> the gripper lowered onto the table top with every body asleep
  (f) the settle of a reset (arm disabled); a Grasp4DofEnv step (finger dynamics)   -> arm_on == 0; no "arm far"
  (g) case (a) in launches of 1, 2, 1, ... substeps -> the masks are per substep: nothing leaks over a launch boundary
"""
import numpy as np
import pytest

from robovat_amd import abi
from test_gpu_env_builds import make_world, _push, _grasp, _record, _replay, _is_hip, _seq_rollout  # noqa: F401
from test_gpu_np_prep import _cfg_of, _counts, _place, BOX

pytestmark = pytest.mark.gpu

N = 32
PAIR01 = abi.RV_MAXB                                          # manifold_counts column of the pair (0, 1)
ARM = slice(abi.RV_MAXB + abi.RV_NBB, abi.RV_MAXB + abi.RV_NBB + abi.RV_MAXB)      # ... of the arm - body manifolds
AWAKE = 8                                                     # env_counters column: awake substeps of the last launch


def _awake(x):
    return np.asarray(x.env_counters())[:, AWAKE]


def _arm_at(x, xyz):
    """The joints put where the gripper points down at xyz (the iteration of test_gpu_np_prep._setup_pushed)."""
    pose = np.tile(np.concatenate([xyz, [1.0, 0.0, 0.0, 0.0]]).astype(np.float32)[None], (N, 1))
    js = np.asarray(x.joint_state()).copy()
    for _ in range(8):
        q = np.asarray(x.compute_ik(pose))
        js[:, :7, 0] = q; js[:, :7, 1] = 0.0
        x.set_joint_state(js)
    return pose


def _push_height(x):
    cfg = _cfg_of(x)
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    return tz, tz + float(cfg.finger_tip_offset) + 0.5 * (float(cfg.cspace_high[2]) + float(cfg.cspace_low[2]))


# ---------------------------------------------------------------------------------------------------------------------
# (a), (b), (g) two sleeping boxes in a row and the scripted push of tests/test_gpu_np_prep.py

RUN = 25                 # substeps per checkpoint
SETTLE = (350, 50)       # the settle: nothing is awake in its second launch
APPROACH = 31            # runs after the target is set in which nothing moves (775 substeps)
RUNS = 40                # ... and all runs (1000 substeps)
SECOND = 0.072           # the second box behind the first (+ 0.001 (i % 4)): a gap of 2 to 5 mm between boxes 7 cm wide -- the
                         # pair manifold of the two sleepers holds points in half of the envs (7.5 cm: in none of them)


def _seq_wake(chunks):
    """chunks: the lengths of the launches a run of RUN substeps is cut into, repeated until it is full."""
    def seq(x, tape):
        x.reset()
        tz, z_push = _push_height(x)
        _arm_at(x, [0.55, 0.0, z_push])
        i = np.arange(N)
        yaw = 0.05 * (i % 8) - 0.15
        first = np.stack([0.64 + 0.002 * (i // 8), 0.004 * (i % 5) - 0.008, np.full(N, tz + 0.031)], 1)
        second = first + np.stack([SECOND + 0.001 * (i % 4), 0 * yaw, 0 * yaw], 1)
        quat = np.stack([0 * yaw, 0 * yaw, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
        _place(x, [(BOX, 0.2, 0.5, first, quat, (0, 0, 0)), (BOX, 0.2, 0.5, second, quat, (0, 0, 0))])
        for k, n in enumerate(SETTLE):
            x.step_sub(n)
            tape(x)
        if not _is_hip(x):
            assert (_awake(x) == 0).all(), _awake(x)                           # everybody sleeps
        rest = np.asarray(x.body_state()).copy()
        end = np.tile(np.array([0.80, 0.0, z_push, 1.0, 0.0, 0.0, 0.0], np.float32)[None], (N, 1))
        x.set_link_target(end)
        woke = np.zeros((N, 2), bool)                    # the box has left its resting pose
        pts_before = np.zeros(N, bool)                   # the pair manifold held points when the first box woke
        mc_prev = _counts(x)
        for run in range(RUNS):
            left, k, awake_sub = RUN, 0, 0
            while left > 0:
                c = min(chunks[k % len(chunks)], left)
                x.step_sub(c); left -= c; k += 1
                awake_sub = awake_sub + _awake(x)
            tape(x)
            if not _is_hip(x):
                st, mc = np.asarray(x.body_state()), _counts(x)
                if run < APPROACH:
                    # the arm is on its way (the frames change) and wake stage 1 runs: it says no, then flags boxes whose
                    # bound has not run out, then queries that miss
                    assert (awake_sub == 0).all() and (st[:, :2] == rest[:, :2]).all(), (run, awake_sub)
                moved = (st[:, :2, :7] != rest[:, :2, :7]).any(2)
                new = moved[:, 0] & ~woke[:, 0]
                pts_before[new] = mc_prev[new, PAIR01] > 0
                woke |= moved
                mc_prev = mc
        if not _is_hip(x):
            assert woke[:, 0].sum() >= N // 2, int(woke[:, 0].sum())          # (a) the arm woke the first box
            both = woke[:, 0] & woke[:, 1]
            # (b) the second box woke too: with the first through the pair manifold where that held points (the island
            # closure), by the moving first box where it held none (the neighbour test of stage 1)
            assert (both & pts_before).sum() >= 2 and (both & ~pts_before).sum() >= 2, (int((both & pts_before).sum()), int((both & ~pts_before).sum()))
    return seq


# ---------------------------------------------------------------------------------------------------------------------
# (c) "arm far": a box slides along the far edge of the table while the arm swings about its base, far from it

def _seq_arm_far(x, tape):
    x.reset()
    tz, z_push = _push_height(x)
    _arm_at(x, [0.45, -0.25, z_push + 0.25])
    i = np.arange(N)
    xyz = np.stack([0.78 + 0.002 * (i % 8), 0.28 + 0.004 * (i // 8), np.full(N, tz + 0.06 + 0.002 * (i % 3))], 1)
    _place(x, [(BOX, 0.2, 0.5, xyz, (0, 0, 0, 1), (0.0, -0.25, 0.0))])
    q = np.asarray(x.joint_state())[:, :abi.RV_NLIMB, 0].astype(np.float32).copy()
    q[:, 0] -= 0.5
    x.set_joint_targets(q)
    lp = np.asarray(x.link_poses()).copy()
    for k in range(4):
        x.step_sub(30)
        tape(x)
        if not _is_hip(x):
            now = np.asarray(x.link_poses())
            # the frames keep changing, the box is awake in every substep and nothing of the arm comes near it
            assert (now[:, 7] != lp[:, 7]).any(1).all() and (_awake(x) == 30).all(), (k, _awake(x))
            assert (_counts(x)[:, ARM] == 0).all()
            d = np.linalg.norm(now[:, :, None, :3] - np.asarray(x.body_state())[:, None, :1, :3], axis=3)
            assert d.min() > 0.3, d.min()
            lp = now.copy()
    x.step_sub(1)        # ... and one more full substep
    tape(x)


# ---------------------------------------------------------------------------------------------------------------------
# (d) arm static: a box dropped in front of the resting gripper

def _seq_arm_static(x, tape):
    x.reset()
    tz, z_push = _push_height(x)
    _arm_at(x, [0.55, 0.0, z_push])
    x.set_joint_targets(np.asarray(x.joint_state())[:, :abi.RV_NLIMB, 0].astype(np.float32).copy())      # (the motors hold that very position)
    i = np.arange(N)
    yaw = 0.07 * (i % 6)
    xyz = np.stack([0.66 + 0.002 * (i // 8), 0.004 * (i % 5) - 0.008, tz + 0.05 + 0.004 * (i % 4)], 1)
    quat = np.stack([0 * yaw, 0 * yaw, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    _place(x, [(BOX, 0.2, 0.5, xyz, quat, (0, 0, 0))])
    x.step_sub(5)
    tape(x)
    js, lp = np.asarray(x.joint_state()).copy(), np.asarray(x.link_poses()).copy()
    for k in range(3):
        x.step_sub(40)
        tape(x)
        if not _is_hip(x):
            # no joint changes by a bit while the box is awake in every substep
            assert (np.asarray(x.joint_state()) == js).all() and (np.asarray(x.link_poses()) == lp).all()
            assert (_awake(x) == 40).all(), _awake(x)


# ---------------------------------------------------------------------------------------------------------------------
# (e) the quiet substep, and the table flags with nobody awake: the gripper is lowered onto the table top

def _seq_quiet_then_table(x, tape):
    x.reset()
    tz, z_push = _push_height(x)
    _arm_at(x, [0.50, 0.0, z_push + 0.05])
    i = np.arange(N)
    xyz = np.stack([0.80 + 0.002 * (i % 8), 0.25 - 0.01 * (i // 8), np.full(N, tz + 0.031)], 1)
    _place(x, [(BOX, 0.2, 0.5, xyz, (0, 0, 0, 1), (0, 0, 0))])
    x.step_sub(350)
    tape(x)
    x.step_sub(40)       # quiet substeps: every body asleep, the resting gripper well above the table
    tape(x)
    if not _is_hip(x):
        assert (_awake(x) == 0).all(), _awake(x)
    i = np.arange(N)
    down = np.tile(np.array([0.50, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], np.float32)[None], (N, 1))
    down[:, 0] += 0.002 * (i % 8); down[:, 2] = tz + float(_cfg_of(x).finger_tip_offset) - 0.02 + 0.001 * (i // 8)
    x.set_link_target(down)
    touched = np.zeros(N, bool)
    for k in range(6):
        x.step_sub(100)
        tape(x)
        if not _is_hip(x):
            assert (_awake(x) == 0).all(), _awake(x)                           # nobody wakes
            touched |= np.asarray(x.query_contacts())[:, 0] > 0                # ... while the arm reaches the table
    if not _is_hip(x):
        assert touched.sum() >= N // 2, int(touched.sum())


def _seq_reset_only(x, tape):
    """reset(): the bodies are dropped and settle with the arm disabled."""
    x.reset()
    tape(x)
    if not _is_hip(x):
        mc = _counts(x)
        assert (mc[:, :abi.RV_MAXB].sum(1) > 0).all() and (mc[:, ARM] == 0).all(), mc


CASES = {
    'a_b_the_arm_wakes_a_sleeper_and_its_neighbour': (_seq_wake((RUN,)), lambda: _push(N, 1)),
    'c_arm_far_with_a_body_awake': (_seq_arm_far, lambda: _push(N, 1)),
    'd_arm_static_with_a_body_awake': (_seq_arm_static, lambda: _push(N, 1)),
    'e_quiet_substeps_then_the_gripper_on_the_table': (_seq_quiet_then_table, lambda: _push(N, 1)),
    'f_settle_with_the_arm_disabled': (_seq_reset_only, lambda: _push(N, 9)),
    'f_finger_dynamics_step': (_seq_rollout((1,), ('env_steps', 'substeps', 'awake_substeps')), lambda: _grasp(N, 7)),
}


@pytest.fixture(scope='module')
def cases():
    done = {}

    def get(name):
        if name not in done:
            seq, make = CASES[name]
            done[name] = _record(seq, *make())
        return done[name]
    return get


@pytest.mark.parametrize('name', sorted(CASES))
def test_light_masks(make_world, cases, name):
    seq, make = CASES[name]
    want = cases(name)
    if name == 'f_finger_dynamics_step':
        cfg, _ = make()
        assert cfg.finger_dynamics == 1 and want[-1]['awake_substeps'] > 0
    _replay(seq, want, make_world, *make())


CUT = (1, 2, 1, RUN)


@pytest.fixture(scope='module')
def cut_case(cases):
    """Case (a) on the oracle with every run of 25 substeps cut into launches of 1, 2, 1 and 21.  The oracle's result
    does not depend on the cut: every checkpoint equals case (a)'s but for the counter columns of the last launch."""
    name = 'a_b_the_arm_wakes_a_sleeper_and_its_neighbour'
    want = _record(_seq_wake(CUT), *CASES[name][1]())
    whole = cases(name)
    assert len(want) == len(whole)
    for a, b in zip(want, whole):
        for key in a:
            assert np.array_equal(a[key][:, :7] if key == 'env_counters' else a[key], b[key][:, :7] if key == 'env_counters' else b[key]), key
    return want


def test_light_masks_cut_into_launches(make_world, cut_case):
    """(g) Case (a) with every run of 25 substeps cut into launches of 1, 2, 1 and 21 substeps: the masks are taken per
    substep, and nothing of them may leak over a launch boundary."""
    _replay(_seq_wake(CUT), cut_case, make_world, *CASES['a_b_the_arm_wakes_a_sleeper_and_its_neighbour'][1]())
