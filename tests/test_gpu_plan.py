"""Planning-mode PushReward on the MI355X (rv_plan_reward / rv_plan_score) against its float32 NumPy restatement
(tests/plan_host.py), bit for bit, on the reference-generated transitions and plans of tests/golden/plan_golden.json;
ties, early termination, the observation as the start state, untouched env state, the parameter checks and the env API."""
import ctypes as C

import numpy as np
import pytest

import plan_host as host
from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu
N = 3
TASKS = ('clearing', 'insertion', 'crossing')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope='module')
def worlds():
    """one world of 3 envs per task x layout, and one without a task"""
    from robovat_amd import lib
    scene, names = scenes.make_scene()
    out = {}
    for task in TASKS + (None,):
        for lid in range(3 if task else 1):
            cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME=task, LAYOUT_ID=lid), n_envs=N,
                                         seed=5, shape_names=names)
            out[(task, lid)] = lib.World(cfg, scene, device=0)
    yield out
    for w in out.values():
        w.close()


def _params(e, nb=None, **kw):
    from robovat_amd import lib
    return lib.plan_params(n_bodies=nb or e['n_bodies'], is_high_level=int(e['is_high_level']), **kw)


def _deal(e, S, H, B):
    """the golden plans of one entry dealt to N envs x S plans (repeated when there are fewer): env n starts where its
    first plan starts, its other plans are moved to that start; H steps and B bodies of each"""
    idx = (np.arange(N * S) % e['count']).reshape(N, S)
    state0 = e['state0'][idx[:, 0]][:, :B]
    shift = state0[:, None] - e['state0'][idx][:, :, :B]
    plans = e['plans'][idx][:, :, :H, :B] + shift[:, :, None]
    return np.ascontiguousarray(state0, np.float32), np.ascontiguousarray(plans, np.float32)


def _score(world, e, state0, plans, gamma=1.0):
    ret, ln, best = world.plan_score(np.array(plans), np.array(state0), _params(e, nb=plans.shape[3], gamma=gamma))      # (copies: the fixture is read-only)
    return ret.cpu().numpy(), ln.cpu().numpy(), best.cpu().numpy()


def test_plan_reward_equals_the_restatement_on_every_golden_transition(worlds):
    g = host.load_golden()
    for e in g['transitions'] + g['strides']:
        w = worlds[(e['task'], e['layout_id'])]
        T = host.Tiles(e['task'], e['layout_id'])
        want_r, want_t = host.plan_reward(T, e['state'], e['next_state'], is_high_level=e['is_high_level'])
        for m in (e['count'], 1, 0):
            r, t = w.plan_reward(e['state'][:m].copy(), e['next_state'][:m].copy(), _params(e))
            assert _same(r.cpu().numpy(), want_r[:m]), (e['task'], e['layout_id'], e['is_high_level'], e['n_bodies'], m)
            assert np.array_equal(t.cpu().numpy().astype(bool), want_t[:m])
        # ... which is the reference's answer (tests/test_plan_reward_golden.py checks the restatement against it)
        assert np.array_equal(want_t, e['termination'])


def test_plan_reward_terms_and_weights(worlds):
    e = next(x for x in host.load_golden()['transitions'] if x['task'] == 'insertion' and x['n_bodies'] == 4)
    w, T = worlds[(e['task'], e['layout_id'])], host.Tiles(e['task'], e['layout_id'])
    for kw in (dict(use_dense_reward=0), dict(use_time_penalty=0), dict(goal_reward=7.5, termination_reward=-3.25, dense_reward=2.5, time_reward=-0.125)):
        r, t = w.plan_reward(e['state'].copy(), e['next_state'].copy(), _params(e, **kw))
        want_r, want_t = host.plan_reward(T, e['state'], e['next_state'], is_high_level=e['is_high_level'], **kw)
        assert _same(r.cpu().numpy(), want_r) and np.array_equal(t.cpu().numpy().astype(bool), want_t)


def test_plan_score_equals_the_reference_recurrence_on_the_golden_plans(worlds):
    """every golden plan with its own start (S = 1): lengths equal the recurrence over the reference's stored flags,
    returns are within H x 5e-5 of it, and both equal the restatement bit for bit"""
    for e in host.load_golden()['plans']:
        w, T = worlds[(e['task'], e['layout_id'])], host.Tiles(e['task'], e['layout_id'])
        ref_ret, ref_len = host.recurrence(e['rewards'], e['terminations'], 0.9)
        for k in range(0, e['count'], N):
            state0, plans = e['state0'][k:k + N], e['plans'][k:k + N, None]
            ret, ln, best = _score(w, e, state0, plans, gamma=0.9)
            h_ret, h_len, h_best = host.plan_score(T, state0, plans, is_high_level=e['is_high_level'], gamma=0.9)
            assert _same(ret, h_ret) and _same(ln, h_len) and _same(best, h_best)
            assert np.array_equal(ln[:, 0], ref_len[k:k + N])
            assert np.max(np.abs(ret[:, 0].astype(np.float64) - ref_ret[k:k + N])) <= e['horizon'] * 5e-5


# S: 1 and 12 deal the golden plans; 63 / 64 / 65 sit around one wave, 257 is the first size of the 16-wave workgroup,
# 1030 makes lanes of that workgroup walk a second plan
@pytest.mark.parametrize('S', [1, 12, 63, 64, 65, 257, 1030])
def test_plan_score_equals_the_restatement(worlds, S):
    lengths_seen = set()
    for e in host.load_golden()['plans']:
        w, T = worlds[(e['task'], e['layout_id'])], host.Tiles(e['task'], e['layout_id'])
        for H in (1, 5):
            for B in (1, 2, 3, 4):
                state0, plans = _deal(e, S, H, B)
                for gamma in (1.0, 0.9):
                    ret, ln, best = _score(w, e, state0, plans, gamma=gamma)
                    h_ret, h_len, h_best = host.plan_score(T, state0, plans, is_high_level=e['is_high_level'], gamma=gamma)
                    key = (e['task'], e['layout_id'], e['is_high_level'], S, H, B, gamma)
                    assert _same(ln, h_len), key
                    assert _same(ret, h_ret), key
                    assert _same(best, h_best), key
                    if H == 5 and B == 4:
                        lengths_seen.update(ln.reshape(-1).tolist())
    assert S < 12 or lengths_seen == {1, 2, 3, 4, 5}


def _one_entry(task='crossing', high=False):
    return next(e for e in host.load_golden()['plans'] if e['task'] == task and e['layout_id'] == 0 and e['is_high_level'] == high)


def test_ties_go_to_the_lowest_index(worlds):
    e = _one_entry()
    w, T = worlds[(e['task'], e['layout_id'])], host.Tiles(e['task'], e['layout_id'])
    ret, _ = host.recurrence(e['rewards'], e['terminations'], 1.0)
    good = int(np.argmax(ret))
    S = 80
    state0 = np.repeat(e['state0'][good][None], N, axis=0)
    plans = np.repeat(np.repeat(state0[:, None, None], e['horizon'], axis=2), S, axis=1)      # nobody moves: the penalty at step 0
    plans[:, 70] = e['plans'][good]
    plans[:, 5] = e['plans'][good]
    h_ret, _, h_best = host.plan_score(T, state0, plans, is_high_level=e['is_high_level'])
    assert h_ret[0, 5] == h_ret[0, 70] and (np.delete(h_ret[0], [5, 70]) < h_ret[0, 5]).all()
    got_ret, _, got_best = _score(w, e, state0, plans)
    assert _same(got_ret, h_ret) and got_best.tolist() == [5] * N and h_best.tolist() == [5] * N
    # (only the higher index: it wins)
    plans[:, 5] = plans[:, 0]
    assert _score(w, e, state0, plans)[2].tolist() == [70] * N


def test_all_plans_ending_at_step_0(worlds):
    e = _one_entry('insertion')
    w, T = worlds[(e['task'], e['layout_id'])], host.Tiles(e['task'], e['layout_id'])
    state0 = np.ascontiguousarray(e['state0'][:N])
    plans = np.repeat(np.repeat(state0[:, None, None], 5, axis=2), 70, axis=1)      # nobody moves: below the minimum stride
    ret, ln, best = _score(w, e, state0, plans)
    h_ret, h_len, h_best = host.plan_score(T, state0, plans, is_high_level=e['is_high_level'])
    assert (ln == 1).all() and _same(ret, h_ret) and best.tolist() == [0] * N


def test_state0_none_is_the_last_observation_and_no_env_state_changes(worlds):
    e = _one_entry('clearing')
    w = worlds[(e['task'], e['layout_id'])]
    w.reset()
    w.set_actions(w.policy_random(0))
    w.step_macro()
    obs = w.observe()['position'][..., :2].contiguous()
    assert float(obs.abs().max()) > 0.1
    before = [w.body_state().cpu().numpy(), w.joint_state().cpu().numpy(), w.env_counters().cpu().numpy()]
    _, plans = _deal(e, 12, 5, 4)
    plans = plans - plans[:, :1, :1] + obs.cpu().numpy()[:, None, None]      # (the walks start near the observation)
    a = w.plan_score(plans, None, _params(e))
    b = w.plan_score(plans, obs, _params(e))
    for x, y in zip(a, b):
        assert _same(x.cpu().numpy(), y.cpu().numpy())
    w.plan_reward(plans[:, :, 0].reshape(-1, 4, 2), plans[:, :, 1].reshape(-1, 4, 2), _params(e))
    after = [w.body_state().cpu().numpy(), w.joint_state().cpu().numpy(), w.env_counters().cpu().numpy()]
    for x, y in zip(before, after):
        assert _same(x, y)


def test_world_without_a_task(worlds):
    w = worlds[(None, 0)]
    e = _one_entry()
    state0, plans = _deal(e, 12, 5, 4)
    r, t = w.plan_reward(plans[0, :, 0], plans[0, :, 1])
    assert (r.cpu().numpy() == 1.0).all() and not t.cpu().numpy().any()
    ret, ln, best = w.plan_score(plans, state0)
    assert (ret.cpu().numpy() == 5.0).all() and (ln.cpu().numpy() == 5).all() and best.cpu().numpy().tolist() == [0] * N


def test_records_that_are_only_8_byte_aligned(worlds):
    """B = 4 reads two float4 per record from a 16-byte aligned buffer and float2 otherwise: the same answers"""
    import torch
    from robovat_amd import lib
    e = _one_entry('insertion', True)
    w = worlds[(e['task'], e['layout_id'])]
    state0, plans = _deal(e, 65, 5, 4)
    want = _score(w, e, state0, plans)
    buf = torch.zeros(plans.size + 2, dtype=torch.float32, device=w.device)
    buf[2:] = torch.as_tensor(plans.reshape(-1), device=w.device)
    view = buf[2:]
    assert view.data_ptr() % 16 == 8
    s0 = torch.as_tensor(state0, device=w.device).contiguous()
    ret = torch.empty((N, 65), dtype=torch.float32, device=w.device)
    ln = torch.empty((N, 65), dtype=torch.int32, device=w.device)
    best = torch.empty((N,), dtype=torch.int32, device=w.device)
    p = _params(e)
    lib.check(w.lib.rv_plan_score(w.h, C.byref(p), w._ptr(s0), w._ptr(view), 65, 5, w._ptr(ret), w._ptr(ln), w._ptr(best)))
    for x, y in zip((ret, ln, best), want):
        assert _same(x.cpu().numpy(), y)
    # returns only / lengths only / best only
    lib.check(w.lib.rv_plan_score(w.h, C.byref(p), w._ptr(s0), w._ptr(view), 65, 5, None, None, w._ptr(best)))
    assert _same(best.cpu().numpy(), want[2])
    ret.zero_()
    lib.check(w.lib.rv_plan_score(w.h, C.byref(p), w._ptr(s0), w._ptr(view), 65, 5, w._ptr(ret), None, None))
    assert _same(ret.cpu().numpy(), want[0])
    with pytest.raises(ValueError):
        lib.check(w.lib.rv_plan_score(w.h, C.byref(p), w._ptr(s0), C.c_void_p(buf.data_ptr() + 4), 65, 5, w._ptr(ret), None, None))


def test_value_errors(worlds):
    import torch
    from robovat_amd import lib
    e = _one_entry()
    w = worlds[(e['task'], e['layout_id'])]
    state0, plans = _deal(e, 12, 5, 4)
    s0, pl = torch.as_tensor(state0, device=w.device), torch.as_tensor(plans, device=w.device)
    ret = torch.empty((N, 12), dtype=torch.float32, device=w.device)
    r = torch.empty((36,), dtype=torch.float32, device=w.device)
    t = torch.empty((36,), dtype=torch.uint8, device=w.device)
    good = _params(e)

    def score(p=good, plans_ptr=w._ptr(pl), s=12, h=5, world=w):
        lib.check(world.lib.rv_plan_score(world.h, None if p is None else C.byref(p), w._ptr(s0), plans_ptr, s, h, w._ptr(ret), None, None))

    def reward(p=good, a=w._ptr(pl), b=w._ptr(pl), m=36, ro=w._ptr(r), to=w._ptr(t)):
        lib.check(w.lib.rv_plan_reward(w.h, None if p is None else C.byref(p), a, b, m, ro, to))
    score(); reward()
    for nb in (0, abi.RV_MAXB + 1, -1):
        with pytest.raises(ValueError):
            score(p=lib.plan_params(n_bodies=nb))
        with pytest.raises(ValueError):
            reward(p=lib.plan_params(n_bodies=nb))
    for kw in (dict(s=0), dict(h=0), dict(s=-3), dict(plans_ptr=None), dict(p=None)):
        with pytest.raises(ValueError):
            score(**kw)
    for kw in (dict(m=-1), dict(a=None), dict(b=None), dict(ro=None), dict(to=None), dict(p=None)):
        with pytest.raises(ValueError):
            reward(**kw)
    # the binding: shapes that disagree
    with pytest.raises(ValueError):
        w.plan_score(plans[:2], state0)
    with pytest.raises(ValueError):
        w.plan_score(plans, state0, lib.plan_params(n_bodies=2))
    with pytest.raises(ValueError):
        w.plan_reward(plans[0, :, 0], plans[0, :, 1, :2])
    with pytest.raises(TypeError):
        lib.plan_params(no_such_field=1)
    # a grasp world has no push task
    env_cfg = configs.grasp_env_config()
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    gw = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=N, shape_names=names), scene, device=0)
    try:
        with pytest.raises(ValueError):
            score(world=gw)
        with pytest.raises(ValueError):
            gw.plan_reward(plans[0, :, 0], plans[0, :, 1])
    finally:
        gw.close()


def test_env_api_takes_xyz_positions():
    import torch
    from robovat_amd.envs.push.push_env import PushEnv, VecPushEnv
    e = _one_entry('insertion')
    T = host.Tiles(e['task'], e['layout_id'])
    cfg = configs.push_env_config(TASK_NAME=e['task'], LAYOUT_ID=e['layout_id'])
    state0, plans = _deal(e, 12, 5, 4)
    h_ret, h_len, h_best = host.plan_score(T, state0, plans, is_high_level=True, gamma=0.9)
    env = VecPushEnv(N, config=cfg)
    try:
        xyz = torch.cat([torch.as_tensor(plans), torch.full(plans.shape[:-1] + (1,), 0.03)], dim=-1)
        s_xyz = np.concatenate([state0, np.full(state0.shape[:-1] + (1,), 0.03, np.float32)], axis=-1)
        for pl, s0 in ((plans, state0), (xyz, s_xyz)):
            ret, ln, best = env.score_plans(pl, s0, is_high_level=True, gamma=0.9)
            assert ret.device == env.device and ret.shape == (N, 12) and ln.shape == (N, 12) and best.shape == (N,)
            assert _same(ret.cpu().numpy(), h_ret) and _same(ln.cpu().numpy(), h_len) and _same(best.cpu().numpy(), h_best)
        r, t = env.plan_rewards(s_xyz, xyz[:, 0, 0])
        want_r, want_t = host.plan_reward(T, state0, plans[:, 0, 0])
        assert t.dtype == torch.bool and _same(r.cpu().numpy(), want_r) and np.array_equal(t.cpu().numpy(), want_t)
    finally:
        env.close()
    one = PushEnv(config=cfg)
    try:
        ret, ln, best = one.score_plans(plans[0], state0[0], is_high_level=True, gamma=0.9)
        assert _same(ret.cpu().numpy(), h_ret[0]) and _same(ln.cpu().numpy(), h_len[0]) and int(best) == int(h_best[0])
        r, t = one.plan_rewards(state0[:1], plans[:1, 0, 0])
        assert _same(r.cpu().numpy(), want_r[:1])
    finally:
        one.close()
