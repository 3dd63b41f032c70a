"""Both builds of the env kernel against the float oracle, in every mode of the env program and with every optional
piece of the physics switched on.

librovat_hip.so holds the env kernel four times (rv_env_kernel.h): the register-rich `k_env` and the 256-register
`k_env_occ2`, each as TMODE = MODE_ROLLOUT and as the run-time-dispatched TMODE = -1.  `k_env_occ2` is what every world
with more envs than the GPU has SIMDs launches, and it is not the same program with fewer registers: the 16 segments of
env_program go through out-of-line seg_* wrappers that rebuild their Consts and reach the env through g_shared, part of
the substep loop lives in scratch, and eight env workgroups share a CU's LDS.  The other GPU tests build worlds of 6 to
96 envs and so run `k_env`; here every case runs on BOTH builds (RV_ENV_OCC forces one on a small world, and
World.env_kernel_build() says which one was launched) and three cases run worlds that fill every CU with eight
workgroups of `k_env_occ2`.

The comparison is bit for bit -- body states, joint states, env counters, manifold sizes and link poses, plus the
stats() keys and observations the case is about: the kernels are written to match the float oracle operation for
operation (no tolerance anywhere in this file).  After a partial step (rv_step_begin / rv_step_poll) the counter
columns 7.. hold the last poll's launch only, so those cases compare the columns [:7].

The oracle's side of a case is computed once per module (fixtures below) and is read-only afterwards.  The seeds and
sizes are those of the one-build tests named in the docstrings; their "this case exercises what it claims" assertions
are kept, on the oracle's data.  Every test is to cost no more than tests/test_gpu_grasp.py::
test_grasp_env_in_partial_batches_equals_the_lock_step (0.6 s on an MI355X), so some cases run fewer steps or envs than
the test they come from; where that is so, the case says it.
"""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes
from test_kat_contact import _Np
from test_gpu_antipodal import NOISE

pytestmark = pytest.mark.gpu

STATE = ('body_state', 'joint_state', 'env_counters', 'manifold_counts', 'link_poses')


def _push(n, seed, offset=0, **over):
    scene, names = scenes.make_scene()
    return configs.make_rv_config(env_cfg=configs.push_env_config(**over), n_envs=n, seed=seed, env_id_offset=offset, shape_names=names), scene


def _grasp(n, seed, offset=0, **over):
    env_cfg = configs.grasp_env_config(**over)
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, env_id_offset=offset, shape_names=names), scene


def _oracle(cfg, scene):
    from oracle import orc
    return orc.OracleWorld(cfg, scene, double=False)


def _freeze(x):
    """The oracle's results are shared by the tests of a case: nobody writes to them."""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)
    return x


def _state(x):
    """The five state arrays of a lib.World (bare or wrapped in _Np) or an OracleWorld, float32 / int32."""
    x = getattr(x, 'w', x)
    out = {}
    for key in STATE:
        a = getattr(x, key)()
        a = a.cpu().numpy() if hasattr(a, 'cpu') else a
        out[key] = a if a.dtype == np.int32 else a.astype(np.float32)
    return out


def _same(got, want, what, rows=slice(None), counters=abi.RV_NCOUNTERS):
    """got[rows] == want, bit for bit, array by array (env counters: the first `counters` columns)."""
    for key in STATE:
        g, w = got[key][rows], want[key]
        if key == 'env_counters':
            g, w = g[:, :counters], w[:, :counters]
        assert g.shape == w.shape, (what, key, g.shape, w.shape)
        bad = np.unique(np.nonzero(g != w)[0])
        assert bad.size == 0, '%s: %s differs in %d envs, first %s' % (what, key, bad.size, bad[:8])


class _Tape(object):
    """Checkpoints of a call sequence.  Run on the oracle it records them; run again with `want` on a HIP world it
    compares every checkpoint with the recorded one: the state arrays and whatever else the sequence hands in."""

    def __init__(self, want=None):
        self.want, self.rows = want, []

    def __call__(self, x, **extra):
        row = _state(x)
        row.update({k: np.asarray(v, np.float64) for k, v in extra.items()})
        if self.want is not None:
            i = len(self.rows)
            ref = self.want[i]
            assert sorted(row) == sorted(ref), (i, sorted(row), sorted(ref))
            _same(row, ref, 'checkpoint %d' % i)
            for k in extra:
                assert np.array_equal(row[k], ref[k]), 'checkpoint %d: %s differs' % (i, k)
        self.rows.append(row)


def _record(seq, cfg, scene):
    tape = _Tape()
    seq(_oracle(cfg, scene), tape)
    assert tape.rows
    return _freeze(tape.rows)


def _is_hip(x):
    return hasattr(x, 'w')


@pytest.fixture(params=['1', '2'], ids=['k_env', 'k_env_occ2'])
def make_world(request, monkeypatch):
    """make(cfg, scene): a lib.World that launches the build this test is about; closed when the test ends."""
    from robovat_amd import lib
    made = []

    def make(cfg, scene):
        assert sum(1 for w in made if w.h) < 2              # (never more than two worlds open)
        monkeypatch.setenv('RV_ENV_OCC', request.param)
        w = lib.World(cfg, scene, device=0)
        made.append(w)
        assert w.env_kernel_build() == int(request.param)
        return w
    yield make
    for w in made:
        w.close()


def _replay(seq, want, make_world, cfg, scene):
    tape = _Tape(want)
    seq(_Np(make_world(cfg, scene)), tape)
    assert len(tape.rows) == len(want)


# ---------------------------------------------------------------------------------------------------------------------
# 1. partial push steps (tests/test_gpu_parity.py::test_partial_batch_trajectories_equal_step_macro: n = 48, seed 41)

@pytest.fixture(scope='module')
def partial_push():
    cfg, scene = _push(48, 41)
    ref = _oracle(cfg, scene)
    ref.reset()
    acts, steps = [], []
    for k in range(2):
        a = ref.policy_random(k)
        ref.set_actions(a); ref.step_macro()
        acts.append(a)
        steps.append(dict(_state(ref), reward=ref.reward()[0].astype(np.float32)))
    return _freeze(dict(acts=acts, steps=steps))


def test_partial_push_steps_in_lock_step(make_world, partial_push):
    """rv_step_begin / rv_step_poll with 700 substeps per launch: the program is resumed mid-step (more than 3 polls
    per step) and after each step every env is where the oracle's step_macro puts it."""
    n = 48
    w = make_world(*_push(n, 41))
    w.reset()
    for k, want in enumerate(partial_push['steps']):
        w.step_begin(partial_push['acts'][k])
        left = np.ones(n, bool); polls = 0
        while left.any():
            fin = w.step_poll(max_substeps=700).cpu().numpy().astype(bool)
            assert not (fin & ~left).any()                        # an env finishes once
            left &= ~fin; polls += 1
            assert polls < 200
        assert polls > 3
        _same(_state(w), want, 'step %d' % k, counters=7)


def test_partial_push_steps_at_each_envs_own_pace(make_world, partial_push):
    """200 us of GPU time per launch, every env restarted as it finishes: the poll buffers' position and reward and
    the state of each finished env are the oracle's after that env's k-th step."""
    import torch
    n, K = 48, len(partial_push['steps'])
    w = make_world(*_push(n, 41))
    w.reset()
    out = w.poll_buffers(point_cloud=True)
    A = torch.as_tensor(np.stack(partial_push['acts']), device='cuda')          # [K, N, G, 4]
    cnt = torch.zeros(n, dtype=torch.long, device='cuda'); ar = torch.arange(n, device='cuda')
    w.step_begin(A[0])
    seen = np.zeros((K, n), bool); polls = 0
    while int(cnt.min()) < K:
        fin = w.step_poll(max_usec=200, out=out).bool()
        polls += 1
        assert polls < 20000
        if not bool(fin.any()):
            continue
        idx = fin.nonzero().flatten().cpu().numpy()
        k_done = cnt.cpu().numpy()[idx]
        got = _state(w)
        pos, rew = out['obs']['position'].cpu().numpy(), out['reward'].cpu().numpy()
        for i, kk in zip(idx, k_done):
            want = partial_push['steps'][kk]
            _same(got, {key: want[key][i:i + 1] for key in STATE}, 'env %d after its step %d' % (i, kk), rows=slice(i, i + 1), counters=7)
            assert np.array_equal(pos[i], want['body_state'][i][:, :3]) and rew[i] == want['reward'][i], (i, kk)
            assert not seen[kk, i]
            seen[kk, i] = True
        cnt[fin] += 1
        nxt = fin & (cnt < K)
        if bool(nxt.any()):
            w.step_begin(A[cnt.clamp(max=K - 1), ar], mask=nxt.to(torch.uint8))
    assert seen.all() and polls > K
    assert np.isfinite(out['obs']['point_cloud'].cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. partial steps with auto-reset (test_gpu_parity.py::test_partial_batches_with_auto_reset: n = 48, seed 43, MAX_STEPS = 2)

def _auto_reset_rounds(ref, acts):
    """The oracle's side of R calls per env with rv_set_auto_reset: step_macro (which skips finished envs), then
    reset(mask = finished before the round).  Per round: the state, who was reset, the observation handed back and which
    envs a body moved in (a body at rest moves only when the arm -- or a body the arm pushed -- touches it)."""
    n = ref.n
    rounds = []
    for k, a in enumerate(acts):
        done_before = ref.reward()[1].astype(bool) if k else np.zeros(n, bool)
        before = ref.body_state()
        ref.set_actions(a); ref.step_macro()
        moved = (np.linalg.norm(ref.body_state()[..., :2] - before[..., :2], axis=-1) > 1e-3).any(-1) & ~done_before
        if done_before.any():
            ref.reset(mask=done_before.astype(np.uint8))
        rounds.append(dict(_state(ref), done_before=done_before, moved=moved, position=ref.observe()[0].astype(np.float32)))
    return rounds


AUTO_RESET_POLLED = slice(16, 32)          # the envs of the 300-substep test


@pytest.fixture(scope='module')
def auto_reset():
    cfg, scene = _push(48, 43, MAX_STEPS=2)
    ref = _oracle(cfg, scene)
    ref.reset()
    acts = [ref.policy_random(k) for k in range(4)]           # step, step, reset, step
    rounds = _auto_reset_rounds(ref, acts)
    assert sum(int(r['done_before'].sum()) for r in rounds) >= 48          # MAX_STEPS = 2: every env was reset at least once
    was_reset = np.cumsum([r['done_before'] for r in rounds], axis=0) > 0
    for rows in (slice(None), AUTO_RESET_POLLED):   # ... every env takes a step AFTER its reset, and in several the arm pushes a body in it
        after = (was_reset[-2] & ~rounds[-1]['done_before'])[rows]
        assert after.all() and (after & rounds[-1]['moved'][rows]).sum() >= 4
    return _freeze(dict(acts=acts, rounds=rounds))


def test_partial_steps_with_auto_reset_round_by_round(make_world, auto_reset):
    """A step begun on a finished episode resets the env -- the reset segments reached from inside a partial step -- and
    the poll hands back what env.reset() returns: reward 0, not done, the reset observation."""
    w = make_world(*_push(48, 43, MAX_STEPS=2))
    w.set_auto_reset(True)
    w.reset()
    out = w.poll_buffers(point_cloud=False)
    for k, want in enumerate(auto_reset['rounds']):
        w.step_begin(auto_reset['acts'][k])
        assert w.step_poll(out=out).cpu().numpy().all()
        _same(_state(w), want, 'round %d' % k, counters=7)
        was = want['done_before']
        d = out['done'].cpu().numpy().astype(bool); r = out['reward'].cpu().numpy()
        assert not d[was].any() and (r[was] == 0).all()
        assert np.array_equal(out['obs']['position'].cpu().numpy()[was], want['position'][was]), k


def test_partial_steps_with_auto_reset_in_300_substep_polls(make_world, auto_reset):
    """The same four calls per env cut into 300-substep polls, envs restarted as they finish: steps, resets with their
    settling runs and the steps that follow a reset, of different envs, in one launch.  Every finished call is checked:
    the env's state, and for a reset the observation, reward 0 and not-done the poll hands back.  (Envs 16 .. 31 of
    the world, made with env_id_offset: a launch lasts as long as its slowest env, and there are 40 and more launches.)"""
    import torch
    lo, n, R = AUTO_RESET_POLLED.start, AUTO_RESET_POLLED.stop - AUTO_RESET_POLLED.start, len(auto_reset['rounds'])
    rounds = [{key: v[AUTO_RESET_POLLED] for key, v in r.items()} for r in auto_reset['rounds']]
    w = make_world(*_push(n, 43, lo, MAX_STEPS=2))
    w.set_auto_reset(True)
    w.reset()
    out = w.poll_buffers(point_cloud=False)
    A = torch.as_tensor(np.stack(auto_reset['acts'])[:, AUTO_RESET_POLLED], device='cuda')
    cnt = torch.zeros(n, dtype=torch.long, device='cuda'); ar = torch.arange(n, device='cuda')
    w.step_begin(A[0]); polls = resets = 0
    while int(cnt.min()) < R:
        fin = w.step_poll(max_substeps=300, out=out).bool()
        polls += 1
        assert polls < 5000
        if bool(fin.any()):
            got = _state(w)
            pos, rew, done = out['obs']['position'].cpu().numpy(), out['reward'].cpu().numpy(), out['done'].cpu().numpy()
            for i, k in zip(fin.nonzero().flatten().cpu().numpy(), cnt.cpu().numpy()[fin.cpu().numpy()]):
                _same(got, {key: rounds[k][key][i:i + 1] for key in STATE}, 'env %d after its call %d' % (i, k), rows=slice(i, i + 1), counters=7)
                if rounds[k]['done_before'][i]:                             # this call was the reset
                    assert np.array_equal(pos[i], rounds[k]['position'][i]) and rew[i] == 0 and not done[i], (i, k)
                    resets += 1
        cnt += fin.long()
        go = fin & (cnt < R)
        if bool(go.any()):
            w.step_begin(A[cnt.clamp(max=R - 1), ar], mask=go.to(torch.uint8))
    assert polls > R and resets >= n


# ---------------------------------------------------------------------------------------------------------------------
# 3. partial grasp steps (tests/test_gpu_grasp.py::test_grasp_env_in_partial_batches_equals_the_lock_step: n = 40, seed 7)

def _grasp_step(ref, a):
    before = ref.body_state()
    ref.set_actions(a); ref.step_macro()
    rr, rd = ref.reward()
    assert rd.all()                                                          # terminate_after_grasp
    moved = np.linalg.norm(ref.body_state()[:, 0, :3] - before[:, 0, :3], axis=-1) > 1e-3
    return dict(_state(ref), reward=rr.astype(np.float32), moved=moved)


@pytest.fixture(scope='module')
def partial_grasp():
    from test_gpu_grasp import _aimed
    cfg, scene = _grasp(40, 7)
    ref = _oracle(cfg, scene)
    ref.reset()
    a = _aimed(ref.body_state(), ref.policy_random(0))
    stepped = _grasp_step(ref, a)
    ref.reset()
    after_reset = _state(ref)
    a2 = _aimed(ref.body_state(), ref.policy_random(1))                     # the grasp of the next episode
    again = _grasp_step(ref, a2)
    assert 1 <= (again['reward'] > 0.5).sum() < 40 and again['moved'].sum() >= 10
    return _freeze(dict(action=a, stepped=stepped, after_reset=after_reset, action2=a2, again=again))


@pytest.mark.parametrize('budget', [dict(max_substeps=137), dict(max_usec=300)], ids=['137_substeps', '300_usec'])
def test_partial_grasp_steps(make_world, partial_grasp, budget):
    """A Grasp4DofEnv step cut mid-phase and mid-wait, by substeps and by GPU time: reward, done, states and the counters
    [:, :7] of the lock step; then, with auto-reset, the begin on the finished episode resets the env, and the grasp of
    the next episode -- a partial step that follows a reset reached from inside a partial step -- ends where the oracle's does."""
    import torch
    n = 40
    w = make_world(*_grasp(n, 7))
    w.reset()
    out = w.poll_buffers(point_cloud=False)
    a = torch.as_tensor(partial_grasp['action']).cuda()

    def step(action, want):
        w.step_begin(action)
        done_mask = np.zeros(n, bool); polls = 0
        rew = np.zeros(n, np.float32)
        while not done_mask.all():
            fin = w.step_poll(out=out, **budget).cpu().numpy().astype(bool)
            assert not (fin & done_mask).any()                               # a step is reported once
            rew[fin] = out['reward'].cpu().numpy()[fin]
            assert out['done'].cpu().numpy()[fin].all()
            done_mask |= fin; polls += 1
            assert polls < 4000
        assert polls > (1 if 'max_usec' not in budget else 0)
        _same(_state(w), want, str(budget), counters=7)
        assert np.array_equal(rew, want['reward'])
    step(a, partial_grasp['stepped'])
    assert not w.step_poll(max_substeps=50).cpu().numpy().any()             # nothing is pending
    w.set_auto_reset(True)
    w.step_begin(a)
    fin = np.zeros(n, bool)
    for _ in range(4000):
        fin |= w.step_poll(max_substeps=500, out=out).cpu().numpy().astype(bool)
        if fin.all():
            break
    assert fin.all()
    _same(_state(w), partial_grasp['after_reset'], 'auto-reset after %s' % budget, counters=7)
    step(torch.as_tensor(partial_grasp['action2']).cuda(), partial_grasp['again'])


# ---------------------------------------------------------------------------------------------------------------------
# 4. entry points that drive the substep loop (tests/test_gpu_entry_points.py at N = 64; test_gpu_scale.py::
#    test_motor_targets_grip_and_reset_targets and tests/test_gpu_sawyer_sim.py for the path, the motor targets and the
#    speed limits)

N_EP = 64


def _top_down(xyz):
    """gripper pose [x, y, z, qx, qy, qz, qw] pointing down (euler [pi, 0, 0]: push_env.py:771)"""
    p = np.zeros((len(xyz), 7), np.float32)
    p[:, :3] = xyz
    p[:, 3] = 1.0
    return p


def _beside(x, b):
    pos = x.body_state()[:, b, :3]
    tz = x.body_params()[:, b, 6]
    return np.stack([pos[:, 0] - 0.07, pos[:, 1], tz + 0.16], axis=1)


def _mid_push(x, tape):
    """Drive the gripper down beside body 0 of every env and then through it: the arm is in contact with the bodies."""
    x.reset()
    start = _beside(x, 0)
    x.set_link_target(_top_down(start)); x.step_sub(900)
    tape(x)
    end = start.copy(); end[:, 0] += 0.16
    x.set_link_target(_top_down(end)); x.step_sub(350)
    return end


def _seq_link_target(x, tape):
    """rv_set_link_target approach and push, rv_query_contacts, rv_compute_ik."""
    end = _mid_push(x, tape)
    flags = x.query_contacts()
    tape(x, contacts=flags)
    assert (np.asarray(flags)[:, 2:].sum(1) > 0).mean() > 0.3               # the arm does touch bodies in a good share of the envs
    assert (np.linalg.norm(x.body_state()[:, 0, 7:10], axis=1) > 0.01).mean() > 0.3
    iks = [x.compute_ik(_top_down(end + np.asarray(d, np.float32))) for d in ([0, 0, 0], [0, 0, 0.12], [0.0, 0.05, 0.03])]
    assert iks[0].shape == (N_EP, abi.RV_NLIMB)
    tape(x, ik=np.stack(iks))                                                # ... and the states are untouched by the queries


def _seq_joint_target_and_waits(x, tape):
    """rv_set_joint_targets retreat mid-push, then rv_wait_until_stable with the defaults of simulator.py:327-331 and
    with the reset thresholds of push_env.py:443-447: states and substep counts."""
    _mid_push(x, tape)
    flags = x.query_contacts()
    assert (np.asarray(flags)[:, 2:].sum(1) > 0).mean() > 0.3
    cfg = getattr(x, 'w', x).cfg
    q = np.tile(np.asarray(cfg.offstage_positions, np.float32)[None, :abi.RV_NLIMB], (N_EP, 1))
    x.set_joint_targets(q); x.step_sub(400)
    tape(x)
    for kw in (dict(lin=0.005, ang=0.005, check_after=100, min_stable=100, max_steps=2000),
               dict(lin=0.1, ang=0.1, check_after=100, min_stable=100, max_steps=500)):
        x.wait_until_stable(**kw)
        s = x.stats()
        assert s['substeps'] >= 199 * N_EP
        tape(x, substeps=s['substeps'], max_substeps=s['max_substeps'])


def _seq_motor_targets_path_and_speed(x, tape):
    """rv_grip + rv_set_motor_targets (position_control_array on two limb joints) on the freshly reset arm, then
    rv_set_link_path (five way points straight down beside body 0) followed at 35 % of the joint speed limits
    (rv_set_max_joint_velocities), then the push through the body at the configured speed."""
    w = getattr(x, 'w', x)
    x.reset()
    js0 = x.joint_state()
    assert np.abs(js0 - js0[:1]).max() == 0.0                               # every arm is reset to the same pose
    joints, delta = [0, 3], [0.2, -0.15]
    q = js0[..., 0].copy()
    for j, d in zip(joints, delta):
        q[:, j] += d
    x.grip(1.0)
    if _is_hip(x):
        mask = np.zeros((N_EP, abi.RV_NJ), np.uint8); mask[:, joints] = 1
        x.set_motor_targets(q.astype(np.float32), mask)
    else:
        x.motor_targets(joints, [float(np.float32(q[0, j])) for j in joints])
    x.step_sub(600)
    js1 = x.joint_state()
    assert (js1[:, 7, 0] < js0[:, 7, 0] - 0.01).all() and (js1[:, 8, 0] > js0[:, 8, 0] + 0.01).all()     # the fingers closed
    assert (np.abs(js1[:, joints, 0] - js0[:, joints, 0]) > 0.05).all()                                # the two joints moved
    tape(x)
    hand = x.link_poses()[:, 7, :3]
    start = _beside(x, 0)
    path = np.stack([_top_down(hand + (start - hand) * (float(i + 1) / 5)) for i in range(5)], axis=1)   # [N, 5, 7]
    vmax = np.asarray([0.35 * float(w.cfg.limb_max_velocity_ratio) * w.scene.arm.v_max[j] for j in range(abi.RV_NLIMB)], np.float32)
    if _is_hip(x):
        x.set_link_path(path)
    else:
        x.set_link_paths(path)
    x.set_max_joint_velocities(vmax)
    x.step_sub(700)
    slow = x.joint_state()
    tape(x)
    # (the speed limit binds: no limb joint is faster than it allows)
    assert (np.abs(slow[:, :abi.RV_NLIMB, 1]) <= vmax[None] * (1 + 1e-5)).all() and np.abs(slow[:, :abi.RV_NLIMB, 1]).max() > 0.5 * vmax.min()
    x.set_link_target(_top_down(start)); x.step_sub(900)
    tape(x)
    end = start.copy(); end[:, 0] += 0.16
    x.set_link_target(_top_down(end)); x.step_sub(350)
    flags = x.query_contacts()
    tape(x, contacts=flags)
    assert (np.asarray(flags)[:, 2:].sum(1) > 0).mean() > 0.3


ENTRY_POINTS = {'link_target': (_seq_link_target, 31), 'joint_target_and_waits': (_seq_joint_target_and_waits, 32),
                'motor_targets_path_and_speed': (_seq_motor_targets_path_and_speed, 33)}


@pytest.fixture(scope='module')
def entry_points():
    return {name: _record(seq, *_push(N_EP, seed)) for name, (seq, seed) in ENTRY_POINTS.items()}


@pytest.mark.parametrize('name', sorted(ENTRY_POINTS))
def test_entry_points(make_world, entry_points, name):
    seq, seed = ENTRY_POINTS[name]
    _replay(seq, entry_points[name], make_world, *_push(N_EP, seed))


# ---------------------------------------------------------------------------------------------------------------------
# 5. limb dynamics, 7. optional physics, 10. rollouts cut into launches: MODE_ROLLOUT with auto-reset

def _seq_rollout(launches, keys):
    def seq(x, tape):
        x.reset()
        tape(x)
        k = 0
        for c in launches:
            x.rollout(c, k, True)
            k += c
            s = x.stats()
            tape(x, **{key: s[key] for key in keys})
    return seq


LIMB = {'PHYSICS.LIMB_DYNAMICS': 1}
LIMB_PUSH = dict(LIMB, MIN_MOVABLE_BODIES=1, MAX_MOVABLE_BODIES=4)
STATS = ('env_steps', 'substeps', 'awake_substeps', 'useful', 'successes')
# name: (config, steps per launch, stats() keys compared, envs that must be reset INSIDE a launch -- counted on the oracle)
ROLLOUTS = {
    # tests/test_limb_dynamics.py::test_limb_dynamics_env_steps_match_the_oracle_bit_for_bit; episodes of two steps, so that
    # the third step follows a reset inside the launch
    'limb_push': (lambda: _push(48, 5, MAX_STEPS=2, **LIMB_PUSH), (3,), STATS, 48),
    # (a grasp step is a whole episode: the second step follows a reset.  12 envs: an object that stays in the gripper keeps
    # the limb rows in the solver through the reward's wait -- env 22 of the 48-env world does so for 15 k awake substeps, a
    # second of GPU time for that one wave; among envs 0 .. 11 one grasp holds and the slowest env has 5.4 k awake substeps)
    'limb_grasp': (lambda: _grasp(12, 5, **LIMB), (2,), STATS, 12),
    # tests/test_limb_dynamics.py::test_lone_limb_island_...: env 73 in its third step of an episode; no reset wanted here
    'lone_limb_island': (lambda: _push(96, 1001, **LIMB_PUSH), (4,), STATS[:3], 0),
    # tests/test_gpu_scale.py::test_rollouts_cut_into_launches_of_any_length_equal_the_oracle
    'cut_into_launches': (lambda: _push(96, 78, MAX_STEPS=2), (1, 2, 1, 3, 1, 1), STATS[:2], 96),
}
# tests/test_gpu_parity.py::test_optional_physics_match_oracle_bit_for_bit: three steps over episodes of two, so that every env
# is reset and settled inside the launch and steps again.  Without deactivation every substep is an awake one: those two
# worlds have 24 envs and take two steps over episodes of one (step, reset and settle, step).
OPTIONAL = [{'PHYSICS.ARM_EFFORT_LIMIT': 1}, {'PHYSICS.GRAVITY_XY': (0.3, -0.2)}, {'PHYSICS.SLEEP_STEPS': 0}, {'PHYSICS.SOLVER_TOL_REST': 1e-7},
            {'PHYSICS.SLEEP_STEPS': 0, 'PHYSICS.SOLVER_TOL_REST': 1e-6, 'MIN_MOVABLE_BODIES': 4, 'MAX_MOVABLE_BODIES': 4}]
for _i, _over in enumerate(OPTIONAL):
    _n, _k = (24, 2) if 'PHYSICS.SLEEP_STEPS' in _over else (48, 3)
    ROLLOUTS['optional_%d' % _i] = (lambda _over=_over, _n=_n, _k=_k: _push(_n, 5, MAX_STEPS=_k - 1, **_over), (_k,), STATS[:3], _n)


@pytest.fixture(scope='module')
def rollouts():
    done = {}

    def get(name):
        if name not in done:
            make, launches, keys, _ = ROLLOUTS[name]
            done[name] = _record(_seq_rollout(launches, keys), *make())
        return done[name]
    return get


@pytest.fixture
def rollout_want(request, rollouts):
    return rollouts(request.node.callspec.params['name'])


@pytest.mark.parametrize('name', sorted(ROLLOUTS))
def test_rollouts(make_world, rollout_want, name):
    make, launches, keys, resets = ROLLOUTS[name]
    want = rollout_want
    assert want[-1]['env_steps'] > 0 and not np.array_equal(want[-1]['body_state'], want[0]['body_state'])
    # num_episodes of the oracle: that many envs began a new episode -- reset and settle -- inside a launch
    assert int((want[-1]['env_counters'][:, 2] > want[0]['env_counters'][:, 2]).sum()) >= resets
    _replay(_seq_rollout(launches, keys), want, make_world, *make())


# ---------------------------------------------------------------------------------------------------------------------
# 6. user constraints (tests/test_constraint.py::test_hip_equals_oracle_with_constraints, n = 6, seed 8, and
#    ::test_hip_equals_oracle_with_a_body_tied_to_a_link, n = 32, seed 17)

def _seq_constraints(x, tape):
    """The six kinds of tests/test_constraint.py::test_hip_equals_oracle_with_constraints, each through a run of substeps
    with the gripper beside body 1: a fixed joint to the world with an offset frame while the arm pushes through the
    body; a point-to-point joint to the world with a fixed joint between two bodies; prismatic joints to the world and
    between bodies with a revolute joint.  (A substep with constraint rows costs about thirty plain ones, so the
    runs are 120 to 150 substeps and the arm is brought up before the first constraint is set.)"""
    x.reset()
    start = _beside(x, 1)
    x.set_link_target(_top_down(start)); x.step_sub(900)
    st = x.body_state()[0]
    tgt = [float(st[1, 0]) + 0.03, float(st[1, 1]) - 0.02, float(st[1, 2]) + 0.05, 0, 0, np.sin(0.2), np.cos(0.2)]
    x.set_constraint(1, tgt, frame7=[0.01, 0, 0.0, 0, 0, 0, 1], max_force=30.0)
    x.step_sub(120)
    tape(x)
    end = start.copy(); end[:, 0] += 0.16
    x.set_link_target(_top_down(end)); x.step_sub(150)                        # a push with the constraint in place
    tape(x, contacts=x.query_contacts())
    x.remove_constraint(1)
    st = x.body_state()[0]
    x.set_constraint(1, [float(st[1, 0]), float(st[1, 1]), float(st[1, 2]) + 0.04, 0, 0, 0, 1], frame7=[0.02, 0.01, 0.0, 0, 0, 0, 1],
                     max_force=30.0, joint_type='point2point')
    x.set_constraint(2, [0.0, 0.0, 0.07, 0, 0, 0, 1], max_force=40.0, child=0)
    x.step_sub(120)
    tape(x)
    st = x.body_state()[0]
    qz = [0, 0, np.sin(0.4), np.cos(0.4)]
    x.remove_constraint(1); x.remove_constraint(2)
    x.set_constraint(1, [float(st[1, 0]), float(st[1, 1]), float(st[1, 2]) + 0.03] + qz, frame7=[0, 0, 0.01] + qz, max_force=60.0, joint_type='prismatic')
    x.set_constraint(3, [0.0, 0.0, 0.08, 0, 0, 0, 1], max_force=40.0, child=0, joint_type='prismatic')
    x.set_constraint(2, [float(st[2, 0]), float(st[2, 1]), float(st[2, 2]) + 0.02] + qz, frame7=[0.015, 0, 0.0] + qz, max_force=50.0, joint_type='revolute')
    x.step_sub(120)
    tape(x)
    if not _is_hip(x):                   # (the bodies moved in every run)
        assert len(tape.rows) == 4 and all(not np.array_equal(tape.rows[i]['body_state'], tape.rows[i + 1]['body_state']) for i in range(3))


def _seq_body_tied_to_a_link(x, tape):
    """tests/test_constraint.py::test_hip_equals_oracle_with_a_body_tied_to_a_link: the arm carries a body by a fixed
    joint to the hand while another swings from a point-to-point joint on a finger link, through a link target; then
    the release.  (Runs of 150 + 150 + 100 substeps, for the cost of constraint rows.)"""
    from test_constraint import _attach_to_hand
    x.reset()
    _attach_to_hand(x, 32)
    lp = x.link_poses()[:, 7]
    x.set_constraint(1, [0.0, 0.0, -0.06, 0, 0, 0, 1], frame7=[0.01, 0.0, 0.02, 0, 0, 0, 1], max_force=80.0, child=abi.RV_CHILD_LINK(8), joint_type='point2point')
    tgt = lp.copy(); tgt[:, 0] += 0.08; tgt[:, 2] -= 0.05
    x.set_link_target(tgt.astype(np.float32))
    for _ in range(2):
        x.step_sub(150)
        tape(x)
    moved = np.linalg.norm(x.link_poses()[:, 7, :3] - lp[:, :3], axis=1)
    assert (moved > 0.01).all()                                             # the hand is on its way, the bodies with it
    held = x.body_state()[:, 0, 2].copy()
    x.remove_constraint(0)
    x.step_sub(100)
    tape(x)
    assert (x.body_state()[:, 0, 2] < held - 0.05).mean() > 0.8              # released: it falls (where no other body is in its way)


CONSTRAINTS = {'to_the_world_and_between_bodies': (_seq_constraints, 6, 8), 'to_an_arm_link': (_seq_body_tied_to_a_link, 32, 17)}


@pytest.fixture(scope='module')
def constraints():
    return {name: _record(seq, *_push(n, seed)) for name, (seq, n, seed) in CONSTRAINTS.items()}


@pytest.mark.parametrize('name', sorted(CONSTRAINTS))
def test_user_constraints(make_world, constraints, name):
    seq, n, seed = CONSTRAINTS[name]
    _replay(seq, constraints[name], make_world, *_push(n, seed))


# ---------------------------------------------------------------------------------------------------------------------
# 8. concentric overlaps (tests/test_gpu_parity.py::test_concentric_overlaps_run_epa_from_a_grown_simplex: n = 64, seed 5)

def _seq_concentric(x, tape):
    x.reset()
    st = x.body_state().copy()
    for a, b in ((0, 1), (2, 3)):
        st[:, b, :7] = st[:, a, :7]
    st[:, :, 2] += 0.03; st[:, :, 7:] = 0
    x.set_body_state(st)
    x.step_sub(1)
    tape(x)
    if not _is_hip(x):                   # the identical-shape pairs hold deep points (the oracle's manifolds)
        same = x.body_params()[:, 0, 1] == x.body_params()[:, 1, 1]
        deep = sum(1 for i in range(64) if same[i] and x.manifold(i, abi.RV_MAXB)[0] > 0 and x.manifold(i, abi.RV_MAXB)[1][:, 9].min() < -0.005)
        assert same.sum() >= 8 and deep == same.sum(), (deep, same.sum())
    x.step_sub(60)
    tape(x)


@pytest.fixture(scope='module')
def concentric():
    return _record(_seq_concentric, *_push(64, 5))


def test_concentric_overlaps(make_world, concentric):
    """The grown-simplex + EPA path of rv_dev_collide.h through the push-out; the pair manifold sizes are part of the
    comparison, the depth of their points is asserted on the oracle's manifolds."""
    _replay(_seq_concentric, concentric, make_world, *_push(64, 5))


# ---------------------------------------------------------------------------------------------------------------------
# 9. recorded observations (tests/test_gpu_scale.py::test_rollout_record_returns_every_steps_observation: n = 24, seed 31)

RECORDED = {'plain': dict(MAX_STEPS=2), 'camera_noise': dict(MAX_STEPS=2, **NOISE)}


@pytest.fixture(scope='module')
def recorded():
    """The oracle in lock step: reset of the finished envs, RandomPolicy action, env.step(), then its observe /
    point_cloud / reward -- what rv_rollout_record has to put into row k."""
    done = {}

    def get(name):
        if name in done:
            return done[name]
        ref = _oracle(*_push(24, 31, **RECORDED[name]))
        ref.reset()
        rows, resets = [], 0
        for k in range(3):
            fin = ref.env_counters()[:, 4].astype(np.uint8)
            if fin.any():
                ref.reset(fin); resets += int(fin.sum())
            ref.set_actions(ref.policy_random(k)); ref.step_macro()
            obs = dict(ref.observe(full=True), point_cloud=ref.point_cloud())
            r, d = ref.reward()
            rows.append(dict(obs=obs, reward=r.astype(np.float32), done=d))
        assert resets >= 24                                                    # MAX_STEPS = 2: the third step follows a reset
        mask = rows[-1]['obs']['body_mask'] > 0
        assert np.abs(rows[-1]['obs']['point_cloud'][mask]).sum() > 0 and (rows[-1]['obs']['point_cloud'][~mask] == 0).all()
        cam = ref.camera().astype(np.float32)
        assert (np.ptp(cam, axis=0).max() > 0) == (name == 'camera_noise')   # every env has a camera of its own, or none has
        done[name] = _freeze(dict(rows=rows, final=_state(ref), camera=cam))
        return done[name]
    return get


@pytest.fixture
def recorded_want(request, recorded):
    return recorded(request.node.callspec.params['name'])


@pytest.mark.parametrize('name', sorted(RECORDED))
def test_recorded_observations(make_world, recorded_want, name):
    """rv_rollout_record with point clouds and every pose modality: row k of every buffer is what the ORACLE observes
    after its k-th step (655 k point clouds per launch of the 8192-env bench line come from this code on k_env_occ2)."""
    want = recorded_want
    w = make_world(*_push(24, 31, **RECORDED[name]))
    w.reset()
    obs, r, d = w.rollout_record(3, first_macro_index=0, auto_reset=True, point_cloud=True, pose_modes=True)
    assert sorted(obs) == sorted(want['rows'][0]['obs'])
    for k, row in enumerate(want['rows']):
        for key in sorted(obs):
            got = obs[key][k].cpu().numpy()
            exp = np.asarray(row['obs'][key]).astype(got.dtype).reshape(got.shape)
            assert np.array_equal(got, exp), (k, key, int((got != exp).sum()))
        assert np.array_equal(r[k].cpu().numpy(), row['reward']), k
        assert np.array_equal(d[k].cpu().numpy(), row['done']), k
    _same(_state(w), want['final'], 'after the recorded rollout', counters=7)
    assert np.array_equal(w.camera().cpu().numpy(), want['camera'])


# ---------------------------------------------------------------------------------------------------------------------
# Co-resident workgroups.  A forced build on a 48-env world puts every workgroup on a CU of its own.  These worlds hold
# 8 x CUs envs (2048 on an MI355X): one full residency of k_env_occ2 -- eight workgroups share every CU's LDS, two waves
# every SIMD -- so a read of an LDS word this launch never wrote sees ANOTHER env's data.  RV_ENV_OCC is not set:
# rv_create picks the build.  Two 32-env slices, the first and the last global ids, are compared with oracle worlds
# made with env_id_offset (the pattern of tests/test_gpu_scale.py::_slice_parity).  The seeds were picked on the CPU
# oracle so that both slices are busy; what "busy" means is asserted below on the oracle's data.

SLICE = 32


def _resident_n():
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _resident(monkeypatch, make_cfg):
    """(world, n, [lo of the two slices]): a world of 8 x CUs envs on the build rv_create picks for it."""
    from robovat_amd import lib
    monkeypatch.delenv('RV_ENV_OCC', raising=False)
    n = _resident_n()
    w = lib.World(*make_cfg(n, 0), device=0)
    return w, n, (0, n - SLICE)


def _busy(moved):
    """Arm-body manifold points in at least a quarter of the slice's envs during the run: a body at rest after the
    reset's settle moves by more than a millimetre only if the arm (or a body the arm pushed) touched it."""
    assert moved.sum() >= SLICE // 4, int(moved.sum())


SEED_PUSH, SEED_GRASP, SEED_LIMB = 9, 21, 5


@pytest.fixture(scope='module')
def resident_push():
    """The two slices of the world below on the oracle, with the oracle's own RandomPolicy actions."""
    n, out = _resident_n(), {}
    for lo in (0, n - SLICE):
        ref = _oracle(*_push(SLICE, SEED_PUSH, lo, MAX_STEPS=1))
        ref.reset()
        acts = [ref.policy_random(k) for k in range(3)]                   # step, reset, step
        rounds = _auto_reset_rounds(ref, acts)
        assert rounds[1]['done_before'].all() and not rounds[2]['done_before'].any()      # every env is reset, then steps again
        _busy(np.any([r['moved'] for r in rounds], axis=0))
        assert rounds[2]['moved'].sum() >= 4                               # ... and the step after the reset pushes bodies too
        out[lo] = dict(acts=np.stack(acts), final=rounds[-1])
    return _freeze(out)


def test_co_resident_partial_push_steps_with_auto_reset(monkeypatch, resident_push):
    """Episodes of one step, three calls per env in 300-substep polls: from the second round rv_step_begin takes a mask
    that restarts only the envs that finished -- the second call resets an env, the third is the step after that reset;
    finished, running and resetting envs share CUs."""
    import torch
    over, R = dict(MAX_STEPS=1), 3
    w, n, los = _resident(monkeypatch, lambda n, lo: _push(n, SEED_PUSH, lo, **over))
    try:
        assert w.env_kernel_build() == abi.RV_ENV_BUILD_OCC2
        w.set_auto_reset(True)
        w.reset()
        A = torch.stack([w.policy_random(k) for k in range(R)])
        cnt = torch.zeros(n, dtype=torch.long, device='cuda'); ar = torch.arange(n, device='cuda')
        w.step_begin(A[0]); polls = 0
        while int(cnt.min()) < R:
            fin = w.step_poll(max_substeps=300).bool()
            polls += 1
            assert polls < 5000
            cnt += fin.long()
            go = fin & (cnt < R)
            if bool(go.any()):
                w.step_begin(A[cnt.clamp(max=R - 1), ar], mask=go.to(torch.uint8))
        assert polls > R
        got, acts = _state(w), A.cpu().numpy()
    finally:
        w.close()
    assert sorted(resident_push) == sorted(los)
    for lo, want in resident_push.items():
        assert np.array_equal(acts[:, lo:lo + SLICE], want['acts'])           # rv_policy_random is keyed by the global env id
        _same(got, want['final'], 'envs %d..' % lo, rows=slice(lo, lo + SLICE), counters=7)


def test_co_resident_partial_grasp_steps(monkeypatch):
    """One Grasp4DofEnv step per env in polls of 137 substeps, every other grasp aimed at the object."""
    from test_gpu_grasp import _aimed
    w, n, los = _resident(monkeypatch, lambda n, lo: _grasp(n, SEED_GRASP, lo))
    try:
        assert w.env_kernel_build() == abi.RV_ENV_BUILD_OCC2
        w.reset()
        a = _aimed(w.body_state().cpu().numpy(), w.policy_random(0).cpu().numpy())
        out = w.poll_buffers(point_cloud=False)
        w.step_begin(a)
        done_mask = np.zeros(n, bool); polls = 0
        rew = np.zeros(n, np.float32)
        while not done_mask.all():
            fin = w.step_poll(max_substeps=137, out=out).cpu().numpy().astype(bool)
            assert not (fin & done_mask).any()
            rew[fin] = out['reward'].cpu().numpy()[fin]
            assert out['done'].cpu().numpy()[fin].all()
            done_mask |= fin; polls += 1
            assert polls < 4000
        assert polls > 1
        got = _state(w)
    finally:
        w.close()
    for lo in los:
        ref = _oracle(*_grasp(SLICE, SEED_GRASP, lo))
        ref.reset()
        assert np.array_equal(a[lo:lo + SLICE], _aimed(ref.body_state(), ref.policy_random(0)))    # the oracle's own actions
        want = _grasp_step(ref, a[lo:lo + SLICE])
        assert 1 <= (want['reward'] > 0.5).sum() < SLICE                      # at least one success and one failure
        _busy(want['moved'])
        _same(got, want, 'envs %d..' % lo, rows=slice(lo, lo + SLICE), counters=7)
        assert np.array_equal(rew[lo:lo + SLICE], want['reward'])


def test_co_resident_limb_dynamics_rollout_with_resets(monkeypatch):
    """Three steps per env in one launch with PHYSICS.LIMB_DYNAMICS and episodes of two steps."""
    over = dict(LIMB_PUSH, MAX_STEPS=2)
    w, n, los = _resident(monkeypatch, lambda n, lo: _push(n, SEED_LIMB, lo, **over))
    try:
        assert w.env_kernel_build() == abi.RV_ENV_BUILD_OCC2
        w.reset()
        w.rollout(3, first_macro_index=0, auto_reset=True, record=False)
        got, stats = _state(w), w.stats()
    finally:
        w.close()
    assert stats['env_steps'] == 3 * n
    for lo in los:
        # the oracle in lock step (reset of the finished envs, action, step), which shows what happened in each step ...
        ref = _oracle(*_push(SLICE, SEED_LIMB, lo, **over))
        ref.reset()
        moved, resets = np.zeros(SLICE, bool), 0
        for k in range(3):
            fin = ref.env_counters()[:, 4].astype(np.uint8)
            if fin.any():
                ref.reset(fin); resets += int(fin.sum())
            before = ref.body_state()
            ref.set_actions(ref.policy_random(k)); ref.step_macro()
            moved |= (np.linalg.norm(ref.body_state()[..., :2] - before[..., :2], axis=-1) > 1e-3).any(-1)
        assert resets >= 1
        _busy(moved)
        _same(got, _state(ref), 'envs %d..' % lo, rows=slice(lo, lo + SLICE), counters=7)
