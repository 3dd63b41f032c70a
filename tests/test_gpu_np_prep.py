"""The preparation of the narrow phase in an awake substep -- the body flag masks, the refresh of the cached points on
one path for the three manifold kinds, the owner / gate lanes, the (body, box) proximity lanes, the work-list masks of
the vertex phase and the owner list the round loop reads (rv_dev_env.h: sim_substep_heavy up to the queries) -- on both
builds of the env kernel against the float oracle, bit for bit: body states, joint states, env counters, manifold
counts and link poses (no tolerance anywhere in this file).

One scene per path of that code, 32 envs each; a scripted scene differs from env to env (offsets and yaw by the env's
index).  Each case first asserts ON THE ORACLE'S DATA that the scene is what it claims, so a scene that stops reaching
its case fails -- without a GPU -- and does not pass empty; the oracle's side of a case is computed once per module
and is read-only afterwards.

  (a) one awake body pushed by the gripper               -> the near mask of its arm-body owner has more than one bit
                                                            and fewer than ten: queries with and without a contact
  (b) a stack of two awake bodies, a sleeper within      -> a pair manifold holds points while other pairs are not live
      the wake range of the lower one
  (c) movables thrown at a static wall                   -> static bits: table / arm manifolds of the wall cleared, pair
                                                            manifolds with it live
  (d) a body beyond the table edge, below the slab       -> the ground manifold path (pair + 64)
  (e) 'crossing' with concave movables                   -> owners of 4 and 16 pairs: several rounds, applies by another group
  (f) the settle of a reset (arm disabled); a Grasp4DofEnv step (finger dynamics)   -> arm_on == 0; no "arm far"
  (g) case (a) in launches of 1, 2, 1, ... substeps      -> the masks are per substep: nothing leaks over a launch boundary
      (case (a) is a scripted push driven by step_sub, not by env steps -- the contact lasts a fraction of one env step --
      so the cut is in SUBSTEPS: every run of 40 as launches of 1, 2, 1 and 36; the oracle is recorded with the same cut)
"""
import numpy as np
import pytest

from robovat_amd import abi
from test_kat_contact import Q0
from test_gpu_env_builds import make_world, _push, _grasp, _oracle, _state, _record, _replay, _is_hip, _seq_rollout  # noqa: F401

pytestmark = pytest.mark.gpu

N = 32
PAIRS = slice(abi.RV_MAXB, abi.RV_MAXB + abi.RV_NBB)          # manifold_counts columns of the six body pairs
ARM0 = abi.RV_MAXB + abi.RV_NBB                               # ... of the arm - body 0 manifold
BOX = 0                                                       # shape 0: the 7 x 7 x 6.2 cm box of tests/test_kat_contact.py


def _counts(x):
    return np.asarray(x.manifold_counts()).astype(np.int64)


def _cfg_of(x):
    return getattr(x, 'w', x).cfg


def _scene_of(x):
    return getattr(x, 'w', x).scene


def _place(x, rows):
    """rows[b] = (shape, mass, friction, xyz [N, 3], quat xyzw [N, 4] or one, vel [N, 3] or one): per-env bodies."""
    p = np.zeros((N, abi.RV_MAXB, 8)); s = np.zeros((N, abi.RV_MAXB, 13)); s[..., 6] = 1
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    for b, (shape, mass, mu, xyz, quat, vel) in enumerate(rows):
        p[:, b] = [1, shape, 1.0, mass, mu, 0, tz, 0]
        s[:, b, :3] = xyz; s[:, b, 3:7] = quat; s[:, b, 7:10] = vel
    x.set_body_params(p); x.set_body_state(s)


def _rot(q):
    """rotation matrices [..., 3, 3] of quaternions xyzw [..., 4]"""
    x, y, z, w = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _near_boxes(x, b, slack):
    """The (body, box) proximity test of the preparation in float64 on the oracle's poses: per env how many collider
    boxes are SURELY near body b (the sphere about the body reaches into the box's AABB by more than `slack`) and how
    many are SURELY not (it stays `slack` short of it)."""
    cfg, arm = _cfg_of(x), _scene_of(x).arm
    shapes = _scene_of(x).shapes
    par, st, lp = np.asarray(x.body_params()), np.asarray(x.body_state()), np.asarray(x.link_poses())
    near = np.zeros(N, int); far = np.zeros(N, int)
    for col in range(abi.RV_NCOL):
        f = int(arm.col_frame[col])
        cc, hh = np.asarray(list(arm.col_center[col])), np.asarray(list(arm.col_half[col]))
        corners = np.array([[cc[0] + sx * hh[0], cc[1] + sy * hh[1], cc[2] + sz * hh[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
        wv = lp[:, f, None, :3] + np.einsum('nij,kj->nki', _rot(lp[:, f, 3:7]), corners)
        lo, hi = wv.min(1), wv.max(1)
        for i in range(N):
            rad = float(shapes[int(par[i, b, 1])].radius) * par[i, b, 2] + float(cfg.margin)
            r = rad + min(float(cfg.breaking) * (rad - float(cfg.margin)), float(cfg.breaking) * float(np.linalg.norm(hh)))
            pos = st[i, b, :3]
            d = np.linalg.norm(np.maximum(lo[i] - pos, 0) + np.maximum(pos - hi[i], 0))
            near[i] += d < r - slack
            far[i] += d > r + slack
    return near, far


# ---------------------------------------------------------------------------------------------------------------------
# (a), (g) one box pushed by the gripper (tests/test_gpu_solver_entry.py case (d) without the second box): the box is
# yawed and off the stroke by amounts that differ from env to env

PUSH_RUN = 40            # substeps per checkpoint
PUSH_RUNS = 8


def _setup_pushed(x):
    cfg = _cfg_of(x)
    x.reset()
    z_push = float(cfg.finger_tip_offset) + 0.5 * (float(cfg.cspace_high[2]) + float(cfg.cspace_low[2]))
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    quat = np.array([1.0, 0.0, 0.0, 0.0])
    start = np.tile(np.concatenate([[0.55, 0.0, tz + z_push], quat]).astype(np.float32)[None], (N, 1))
    end = np.tile(np.concatenate([[0.75, 0.0, tz + z_push], quat]).astype(np.float32)[None], (N, 1))
    js = np.asarray(x.joint_state()).copy()
    for _ in range(8):
        q = np.asarray(x.compute_ik(start))
        js[:, :7, 0] = q; js[:, :7, 1] = 0.0
        x.set_joint_state(js)
    i = np.arange(N)
    yaw = 0.05 * (i % 8) - 0.15
    xyz = np.stack([0.62 + 0.002 * (i // 8), 0.004 * (i % 5) - 0.008, np.full(N, tz + 0.031)], 1)
    quat = np.stack([0 * yaw, 0 * yaw, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    _place(x, [(BOX, 0.2, 0.5, xyz, quat, (0, 0, 0))])
    x.set_link_target(end)
    return xyz


def _seq_pushed(chunks):
    """chunks: the lengths of the launches a run of PUSH_RUN substeps is cut into, repeated until it is full."""
    def seq(x, tape):
        xyz = _setup_pushed(x)
        without, with_ = np.zeros(N, bool), np.zeros(N, bool)
        awake_sub = 0
        for _ in range(PUSH_RUNS):
            left, k = PUSH_RUN, 0
            while left > 0:
                c = min(chunks[k % len(chunks)], left)
                x.step_sub(c); left -= c; k += 1
                awake_sub += np.asarray(x.env_counters())[:, 8]               # awake substeps of this launch
            tape(x)
            if not _is_hip(x):
                mc = _counts(x)
                assert (mc[:, PAIRS] == 0).all() and (mc[:, 1:abi.RV_MAXB] == 0).all(), mc       # one body
                near, far = _near_boxes(x, 0, 2e-3)
                # at least two boxes (the fingers) are near the box and at least one (a link of the limb) is not: the
                # near mask of its arm-body owner has more than one bit and fewer than ten
                partial = (near >= 2) & (far >= 1)
                without |= partial & (mc[:, ARM0] == 0)
                with_ |= partial & (mc[:, ARM0] > 0)
        if not _is_hip(x):
            # the box was awake in every substep (it is put down a hair above the table and pushed before it can sleep), so
            # its arm-body owner was live throughout: with boxes near it ran queries that found no contact (no point in
            # the manifold yet) and later queries that did
            assert (awake_sub == PUSH_RUN * PUSH_RUNS).all(), awake_sub
            assert without.sum() >= N // 2 and with_.sum() >= N // 2, (int(without.sum()), int(with_.sum()))
            assert (np.asarray(x.body_state())[:, 0, 0] > xyz[:, 0] + 0.01).all()       # the box was pushed along
    return seq


# ---------------------------------------------------------------------------------------------------------------------
# (b) a stack of two boxes beside a third box that has gone to sleep

def _seq_stack_beside_a_sleeper(x, tape):
    x.reset()
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    i = np.arange(N)
    z0 = tz + 0.031
    base = np.stack([0.6 + 0.001 * (i % 4), 0.002 * (i // 4) - 0.008, np.full(N, z0)], 1)
    top = base + np.stack([0.005 + 0.0005 * (i % 7), 0.003 - 0.0004 * (i % 3), np.full(N, 0.062 + 0.08)], 1)
    third = base + [0.0, 0.11, 0.0]
    # the third box rests from the start, 4 cm beside the first, and sleeps after about 205 substeps; the second is dropped
    # from 8 cm onto the first and keeps the stack awake until about substep 325
    _place(x, [(BOX, 0.3, 0.5, base, Q0, (0, 0, 0)), (BOX, 0.2, 0.5, top, Q0, (0, 0, 0)), (BOX, 0.3, 0.5, third, Q0, (0, 0, 0))])
    x.step_sub(230)
    tape(x)
    prev = np.asarray(x.body_state()).copy()
    ok = np.ones(N, bool)
    for k in range(3):
        x.step_sub(30)
        tape(x)
        if not _is_hip(x):
            mc = _counts(x)
            st = np.asarray(x.body_state())
            # pair 0 = bodies (0, 1) holds points and the stack is awake in every substep of the launch, while body 2 does not
            # move by a bit -- it is asleep -- and the pairs with it (1 and 3) are not live.  The sleeper is within the wake
            # range of body 0 (the wake test of sim_substep_light: centres closer than radius + radius + brk_bb; only a
            # neighbour that has left its pose window wakes a sleeper, and body 0 under the falling box has not)
            assert (mc[:, [abi.RV_MAXB + 1, abi.RV_MAXB + 3]] == 0).all(), (k, mc)
            cfg = _cfg_of(x)
            rad = float(_scene_of(x).shapes[BOX].radius) + float(cfg.margin)
            assert (np.linalg.norm(st[:, 0, :3] - st[:, 2, :3], axis=1) < 2 * rad + float(cfg.breaking) * (rad - float(cfg.margin)) - 1e-3).all()
            ok &= (mc[:, abi.RV_MAXB + 0] > 0) & (np.asarray(x.env_counters())[:, 8] == 30) & (st[:, 2] == prev[:, 2]).all(1)
            ok &= (np.abs(st[:, 1, 7:]).max(1) > 0)
            prev = st.copy()
    if not _is_hip(x):
        assert ok.sum() >= N // 2, int(ok.sum())


# ---------------------------------------------------------------------------------------------------------------------
# (c) a static wall (tests/test_static_body.py: WALLS[0]), the movables thrown at it

WALL = {'SIM.WALL.USE': True, 'SIM.WALL.POSE': [[0.66, 0.0, 0.4], [0, 0, 0]], 'MAX_MOVABLE_BODIES': 3, 'MIN_MOVABLE_BODIES': 3}
WALL_SLOT = abi.RV_MAXB - 1
WALL_PAIRS = [abi.RV_MAXB + 2, abi.RV_MAXB + 4, abi.RV_MAXB + 5]     # pairs (0, 3), (1, 3), (2, 3)


def _seq_wall(x, tape):
    from test_static_body import _throw_at_the_wall
    x.reset()
    tape(x)
    par = np.asarray(x.body_params())
    x.set_body_state(_throw_at_the_wall(_cfg_of(x), np.asarray(x.body_state()), par))
    hit = np.zeros(N, bool)
    for _ in range(4):
        x.step_sub(60)
        tape(x)
        if not _is_hip(x):
            mc = _counts(x)
            assert (par[:, WALL_SLOT, 0] == 1).all() and (par[:, WALL_SLOT, 3] == 0).all()      # the wall: present, mass 0
            assert (mc[:, WALL_SLOT] == 0).all() and (mc[:, ARM0 + WALL_SLOT] == 0).all()       # no table / arm manifold
            hit |= (mc[:, WALL_PAIRS] > 0).any(1)
    if not _is_hip(x):
        assert hit.sum() >= N // 2, int(hit.sum())                           # pair manifolds with the wall hold points


# ---------------------------------------------------------------------------------------------------------------------
# (d) a box beyond the table's edge and below its slab: it lands on the ground

def _seq_ground(x, tape):
    cfg = _cfg_of(x)
    x.reset()
    i = np.arange(N)
    gz = float(cfg.ground_z)
    yaw = 0.1 * (i % 6)
    xyz = np.stack([1.3 + 0.01 * (i % 4), 0.02 * (i // 8), gz + 0.06 + 0.004 * (i % 5)], 1)
    quat = np.stack([0 * yaw, 0 * yaw, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1)
    _place(x, [(BOX, 0.2, 0.5, xyz, quat, (0.05, 0, 0))])
    tz = float(np.asarray(x.body_params())[0, 0, 6])
    assert (xyz[:, 2] + 0.1 < tz - float(cfg.table_thickness)).all()          # below the slab from the first substep on
    for k in range(4):
        x.step_sub(80)
        tape(x)
    if not _is_hip(x):
        mc = _counts(x)
        st = np.asarray(x.body_state())
        # the "table" manifold of the body holds its contacts with the ground
        assert (mc[:, 0] > 0).all() and (np.abs(st[:, 0, 2] - (gz + 0.031)) < 5e-3).all(), (mc[:, 0], st[:, 0, 2])


# ---------------------------------------------------------------------------------------------------------------------
# (e) concave movables, (f) no arm / finger dynamics

CONCAVE = dict(TASK_NAME='crossing', LAYOUT_ID=0, MOVABLE_NAME='CONCAVE')
BB = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]        # the bodies of pair k (rv_dev_env_types.h: bb_a, bb_b)


def _seq_concave(x, tape):
    x.reset()
    tape(x)
    shapes = _scene_of(x).shapes
    four, sixteen = 0, 0
    for k in range(2):
        x.rollout(1, k, True)
        tape(x)
        if not _is_hip(x):
            mc, par = _counts(x), np.asarray(x.body_params())
            hulls = np.array([[int(shapes[int(par[i, b, 1])].n_hulls) * int(par[i, b, 0]) for b in range(abi.RV_MAXB)] for i in range(N)])
            # a body of four hulls on the table: an owner of 4 pairs (one round).  Two such bodies whose pair manifold holds
            # points: an owner of 16 pairs -- four rounds.  "Applied by another group" follows from the counts, it is not
            # observed: the results of one manifold in a round are applied by the group that holds the first of them, so every
            # owner with two or more pairs in a round -- each of these -- has results of groups 1 .. 3 applied by another one
            four += int(((hulls == 4) & (mc[:, :abi.RV_MAXB] > 0)).sum())
            for p, (a, b) in enumerate(BB):
                sixteen += int(((hulls[:, a] * hulls[:, b] == 16) & (mc[:, abi.RV_MAXB + p] > 0)).sum())
    if not _is_hip(x):
        assert four >= N and sixteen >= 2, (four, sixteen)


def _seq_reset_only(x, tape):
    """reset(): the bodies are dropped and settle with the arm disabled -- every heavy substep has arm_on == 0."""
    x.reset()
    tape(x)
    if not _is_hip(x):
        mc = _counts(x)
        assert (mc[:, :abi.RV_MAXB].sum(1) > 0).all() and (mc[:, ARM0:] == 0).all(), mc


CASES = {
    'a_partial_near_mask': (_seq_pushed((PUSH_RUN,)), lambda: _push(N, 1)),
    'b_pair_manifold_beside_a_sleeper': (_seq_stack_beside_a_sleeper, lambda: _push(N, 1)),
    'c_static_wall': (_seq_wall, lambda: _push(N, 3, **WALL)),
    'd_ground_manifold': (_seq_ground, lambda: _push(N, 1)),
    'e_concave_owners_of_4_and_16_pairs': (_seq_concave, lambda: _push(N, 27, MAX_STEPS=3, **CONCAVE)),
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
def test_np_prep(make_world, cases, name):
    seq, make = CASES[name]
    want = cases(name)
    if name == 'f_finger_dynamics_step':
        cfg, _ = make()
        # the force-limited gripper: no "arm far" substeps; the grasp moves the object in a good share of the envs
        assert cfg.finger_dynamics == 1 and want[-1]['awake_substeps'] > 0
        assert (np.abs(want[-1]['body_state'][:, 0, :3] - want[0]['body_state'][:, 0, :3]).max(1) > 1e-3).sum() >= N // 4
    _replay(seq, want, make_world, *make())


CUT = (1, 2, 1, PUSH_RUN)


@pytest.fixture(scope='module')
def cut_case(cases):
    """Case (a) on the oracle in launches of 1, 2, 1 and 36 substeps per run of 40.  The oracle's result does not depend
    on the cut: every checkpoint equals case (a)'s but for the counter columns that hold the last launch only."""
    _, make = CASES['a_partial_near_mask']
    want = _record(_seq_pushed(CUT), *make())
    whole = cases('a_partial_near_mask')
    assert len(want) == len(whole)
    for a, b in zip(want, whole):
        for key in a:
            assert np.array_equal(a[key][:, :7] if key == 'env_counters' else a[key], b[key][:, :7] if key == 'env_counters' else b[key]), key
    return want


def test_np_prep_cut_into_launches(make_world, cut_case):
    """(g) The push of case (a) with every run of 40 substeps cut into launches of 1, 2, 1 and 36 substeps: the masks
    are taken per substep, and nothing of them may leak over a launch boundary."""
    _, make = CASES['a_partial_near_mask']
    _replay(_seq_pushed(CUT), cut_case, make_world, *make())
