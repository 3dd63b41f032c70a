"""The entry of the solver in an awake substep -- the awake / coupling masks, the uncoupled fast path, the contact flags,
the Delassus columns of solve_singles (rv_dev_env.h: sim_substep_heavy between the narrow phase and the sweeps) -- on
both builds of the env kernel against the float oracle, bit for bit: body states, joint states, env counters, manifold
counts and link poses (no tolerance anywhere in this file).

One scene per path of that code.  Each case first asserts ON THE ORACLE'S DATA that the scene is what it claims (which
manifolds hold points while it runs), so a wrong scene fails without a GPU; the oracle's side of a case is computed
once per module and is read-only afterwards.

  (a) four awake bodies, no pair manifold with points     -> uncoupled fast path, smask = 15
  (b) a stack of two boxes                                -> general path, solve_island2
  (c) a stack of three boxes                              -> general path, the island of three or four bodies
  (d) a pushed box beside a second awake body             -> fast path with arm rows, fewer than four arm points
  (e) a recorded rollout with auto-reset                  -> the paths alternate; the flags feed check_safety
  (f) Grasp4DofEnv, one body                              -> finger dynamics rule the fast path out: solve_island_fingers
  (g) a user constraint on an awake body among four       -> rows_all: the row-setup phase scales the kept impulses, the
                                                             one-lane system solver takes every row
"""
import numpy as np
import pytest

from robovat_amd import abi
from test_kat_contact import _bodies, Q0
from test_gpu_env_builds import make_world, _push, _grasp, _oracle, _state, _same, _freeze, _record, _replay, _is_hip, _seq_rollout  # noqa: F401

pytestmark = pytest.mark.gpu

PAIRS = slice(abi.RV_MAXB, abi.RV_MAXB + abi.RV_NBB)          # manifold_counts columns of the six body pairs
ARM0 = abi.RV_MAXB + abi.RV_NBB                               # ... of the arm - body 0 manifold


def _counts(x):
    return np.asarray(x.manifold_counts()).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# (a) uncoupled, several bodies

def _cfg_uncoupled():
    return _push(8, 3, **{'PHYSICS.SLEEP_STEPS': 0, 'MIN_MOVABLE_BODIES': 4, 'MAX_MOVABLE_BODIES': 4})


def _seq_uncoupled(x, tape):
    x.reset()
    tape(x)
    for _ in range(3):
        x.step_sub(50)
        tape(x)
        if not _is_hip(x):
            # four bodies, none asleep (no deactivation), each on the table, no pair manifold with points
            assert (np.asarray(x.body_params())[:, :, 0] == 1).all()
            mc = _counts(x)
            assert (mc[:, PAIRS] == 0).all() and (mc[:, :abi.RV_MAXB] > 0).all(), mc
    if not _is_hip(x):
        s = x.stats()
        assert s['awake_substeps'] == s['substeps'] > 0


# ---------------------------------------------------------------------------------------------------------------------
# (b), (c) stacks of two and three boxes (tests/test_kat_contact.py::test_two_box_stack_rests)

Z0 = 0.031
STACK = [(0, 0.3, 0.5, (0.6, 0.0, Z0), Q0, (0, 0, 0)), (0, 0.2, 0.5, (0.605, 0.003, Z0 + 0.062), Q0, (0, 0, 0)),
         (0, 0.15, 0.5, (0.602, -0.002, Z0 + 0.124), Q0, (0, 0, 0))]


def _seq_stack(boxes):
    def seq(x, tape):
        _bodies(x, STACK[:boxes], n=4)
        for k in range(4):
            x.step_sub(50)
            tape(x)
            if not _is_hip(x):
                mc = _counts(x)
                # pair 0 = bodies (0, 1), pair 3 = bodies (1, 2): the islands are the whole stack
                assert (mc[:, abi.RV_MAXB + 0] > 0).all(), (k, mc)
                assert (mc[:, 0] > 0).all() and (mc[:, 1] == 0).all()
                if boxes == 3:
                    assert (mc[:, abi.RV_MAXB + 3] > 0).all() and (mc[:, 2] == 0).all(), (k, mc)
        if not _is_hip(x):
            st = np.asarray(x.body_state())
            assert np.abs(st[:, :boxes, 2] - [r[3][2] for r in STACK[:boxes]]).max() < 4e-3       # the stack stands
    return seq


# ---------------------------------------------------------------------------------------------------------------------
# (d) a pushed body with arm points beside a second awake body (tests/test_kat_contact.py::
#     test_pushed_box_moves_with_the_pusher, with the box yawed and a second box dropped 13 cm to the side; no
#     deactivation, so that the second box is awake for the whole push)

def _cfg_pushed():
    return _push(4, 1, **{'PHYSICS.SLEEP_STEPS': 0})


def _seq_pushed(x, tape):
    cfg = getattr(x, 'w', x).cfg
    n = 4
    x.reset()
    z_push = float(cfg.finger_tip_offset) + 0.5 * (float(cfg.cspace_high[2]) + float(cfg.cspace_low[2]))
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    quat = np.array([1.0, 0.0, 0.0, 0.0])
    start = np.tile(np.concatenate([[0.55, 0.0, tz + z_push], quat]).astype(np.float32)[None], (n, 1))
    end = np.tile(np.concatenate([[0.75, 0.0, tz + z_push], quat]).astype(np.float32)[None], (n, 1))
    js = np.asarray(x.joint_state()).copy()
    for _ in range(8):
        q = np.asarray(x.compute_ik(start))
        js[:, :7, 0] = q; js[:, :7, 1] = 0.0
        x.set_joint_state(js)
    p = np.zeros((n, abi.RV_MAXB, 8)); s = np.zeros((n, abi.RV_MAXB, 13)); s[..., 6] = 1
    # (the box yawed by 0.3 rad and 2 cm off the stroke: a finger meets an edge of it -- two arm points, not four)
    p[:, 0] = [1, 0, 1.0, 0.2, 0.5, 0, tz, 0]; s[:, 0, :3] = [0.62, 0.02, tz + 0.031]; s[:, 0, 3:7] = [0, 0, np.sin(0.15), np.cos(0.15)]
    p[:, 1] = [1, 0, 1.0, 0.2, 0.5, 0, tz, 0]; s[:, 1, :3] = [0.62, 0.15, tz + 0.06]        # dropped from 3 cm
    x.set_body_params(p); x.set_body_state(s)
    x.set_link_target(end)
    touching = []
    for _ in range(8):
        x.step_sub(40)
        tape(x)
        if not _is_hip(x):
            mc = _counts(x)
            assert (mc[:, PAIRS] == 0).all(), mc                       # the two boxes never meet
            touching.append(mc[:, ARM0].copy())
    if not _is_hip(x):
        touching = np.array(touching)
        # the arm manifold of the pushed box holds one to three points at several checkpoints, in every env, while the
        # second box is awake on the table beside it
        assert ((touching > 0) & (touching < 4)).sum(0).min() >= 2, touching
        assert (_counts(x)[:, 1] > 0).all()
        assert (np.asarray(x.body_state())[:, 0, 0] > 0.62 + 0.01).all()       # the box was pushed along


# ---------------------------------------------------------------------------------------------------------------------
# (e) recorded rollout with auto-reset, (f) finger dynamics, (g) a user constraint

def _cfg_recorded():
    return _push(16, 5, MAX_STEPS=2)


@pytest.fixture(scope='module')
def recorded_rollout():
    ref = _oracle(*_cfg_recorded())
    ref.reset()
    first = _state(ref)
    ref.rollout(3, 0, True)
    r, d = ref.reward()
    final = _state(ref)
    # episodes of two steps: every env was reset inside the rollout and stepped again; bodies moved
    assert (final['env_counters'][:, 2] > first['env_counters'][:, 2]).all()
    assert not np.array_equal(final['body_state'], first['body_state'])
    return _freeze(dict(final=final, reward=r.astype(np.float32), done=np.asarray(d), substeps=ref.stats()['substeps']))


def _cfg_fingers():
    return _grasp(8, 7)


# (g) four awake bodies on the table (no deactivation); body 1 is tied by a fixed joint to a frame 5 cm above where it
#     rests.  An awake body with a constraint and no limb rows is rows_all: in every substep the kept impulses of ALL
#     manifolds with points are scaled by the row-setup phase and the system solver solves them.  (A substep with
#     constraint rows costs about thirty plain ones: 4 envs, 90 substeps.)

def _cfg_constraint():
    return _push(4, 3, **{'PHYSICS.SLEEP_STEPS': 0, 'MIN_MOVABLE_BODIES': 4, 'MAX_MOVABLE_BODIES': 4})


def _seq_constraint(x, tape):
    x.reset()
    st0 = np.asarray(x.body_state()).copy()
    tgt = [float(st0[0, 1, 0]), float(st0[0, 1, 1]), float(st0[0, 1, 2]) + 0.05, 0, 0, 0, 1]
    x.set_constraint(1, tgt, max_force=30.0)
    for _ in range(3):
        x.step_sub(30)
        tape(x)
        if not _is_hip(x):
            mc = _counts(x)
            # the other three bodies rest on the table with points in their manifolds (impulses are kept and scaled)
            assert (mc[:, [0, 2, 3]] > 0).all(), mc
    if not _is_hip(x):
        s = x.stats()
        assert s['awake_substeps'] == s['substeps'] > 0                  # body 1 was awake in every substep ...
        st = np.asarray(x.body_state())
        # ... and only the constraint lifts a body off the table: its rows were in the solve (env 0 reaches the target's
        # height; the constraint is per world, so the other envs are pulled towards env 0's frame as well)
        assert st[0, 1, 2] > st0[0, 1, 2] + 0.03, (st[0, 1, 2], st0[0, 1, 2])
        assert (np.linalg.norm(st[:, 1, :3] - st0[:, 1, :3], axis=1) > 0.01).all()


CASES = {
    'a_uncoupled_four_bodies': (_seq_uncoupled, _cfg_uncoupled),
    'b_two_body_island': (_seq_stack(2), lambda: _push(4, 1)),
    'c_three_body_island': (_seq_stack(3), lambda: _push(4, 1)),
    'd_pushed_body_beside_an_awake_one': (_seq_pushed, _cfg_pushed),
    'f_finger_dynamics_one_body': (_seq_rollout((2,), ('env_steps', 'substeps', 'awake_substeps')), _cfg_fingers),
    'g_user_constraint_rows_all': (_seq_constraint, _cfg_constraint),
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
def test_solver_entry(make_world, cases, name):
    seq, make = CASES[name]
    want = cases(name)
    if name == 'f_finger_dynamics_one_body':
        cfg, _ = make()
        # one body and the force-limited gripper: never the uncoupled fast path, never rows_all (fing_fast)
        assert cfg.finger_dynamics == 1 and (want[-1]['body_state'][:, 1:, :3] == want[0]['body_state'][:, 1:, :3]).all()
        assert want[-1]['awake_substeps'] > 0 and not np.array_equal(want[-1]['body_state'], want[0]['body_state'])
    _replay(seq, want, make_world, *make())


def test_recorded_rollout_with_auto_reset(make_world, recorded_rollout):
    """Three recorded steps over episodes of two: envs alternate between the paths from substep to substep, and the
    contact flags of every substep feed check_safety -- a wrong flag ends an episode the oracle goes on with."""
    want = recorded_rollout
    w = make_world(*_cfg_recorded())
    w.reset()
    obs, r, d = w.rollout_record(3, first_macro_index=0, auto_reset=True, point_cloud=False)
    _same(_state(w), want['final'], 'after the recorded rollout')
    assert w.stats()['substeps'] == want['substeps']
    assert np.array_equal(r[-1].cpu().numpy(), want['reward'])
    assert np.array_equal(d[-1].cpu().numpy().astype(bool), want['done'].astype(bool))
