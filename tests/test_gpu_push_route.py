"""rv_get_route_field / rv_policy_route_multi / rv_plan_propose_route and RouteShootingPushPolicy on the MI355X.  The
field is compared with the queue BFS of tests/push_route_host.py, the proposal kernel bit for bit with that file's float32
restatement of csrc/rv_dev_push_route.h fed with what the world observes; rv_plan_propose_route and the policy with the
same loops made of separate calls.  Worlds of 2 to 15 envs."""
import ctypes as C

import numpy as np
import pytest

import push_route_host as host
from robovat_amd import abi, configs, lib, scenes

pytestmark = pytest.mark.gpu
F = np.float32
N, OFFSET, S, SEED = 3, 5, 5, 17 + (3 << 32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _np(x):
    return x.cpu().numpy()


def _cfg(n, offset=0, task='crossing', layout=0):
    scene, names = scenes.make_scene()
    env_cfg = configs.push_env_config(TASK_NAME=task, LAYOUT_ID=layout, MAX_STEPS=3)
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, shape_names=names, env_id_offset=offset, seed=SEED), scene


def _world(n, offset=0, task='crossing', layout=0, edit=None):
    cfg, scene = _cfg(n, offset, task, layout)
    if edit is not None:
        edit(cfg)
    return lib.World(cfg, scene, device=0)


FIELDS = [(t, l, None) for t in ('crossing', 'insertion') for l in range(3)] + [('crossing', 0, 'WRAP'), ('crossing', 0, 'ISLAND')]


@pytest.mark.parametrize('task,layout,tiles', FIELDS)
def test_route_field_equals_the_host_bfs(task, layout, tiles):
    # (the synthetic tiles: the ctypes rv_config edited before the world is made)
    w = _world(2, task=task, layout=layout, edit=(lambda cfg: host.set_tiles(cfg, *getattr(host, tiles))) if tiles else None)
    try:
        d = _np(w.route_field())
        assert d.shape == (8, 8) and d.dtype == np.uint8
        assert np.array_equal(d.reshape(64), host.route_field(w.cfg))
        assert np.array_equal(_np(w.route_field()), d)      # the kept field, again
        assert (d != 255).any() and (d == 0).sum() == w.cfg.n_goal
    finally:
        w.close()


def _want(world, s, offset=0, **kw):
    """the restatement on what `world` observes now -> (actions [M, s, G, 4], status [M, s])"""
    pos, nb, mov = host.world_inputs(world.observe())
    a, st = host.proposals(host.Route(world.cfg), pos, nb, mov, SEED, offset, s, host.params(**kw))
    return np.ascontiguousarray(np.broadcast_to(a[:, :, None, :], (a.shape[0], s, world.G, 4))), st


def _got(world, s, **kw):
    a, st = world.policy_route_multi(lib.push_route_params(**kw), s)
    return _np(a), _np(st)


def _place(world, xy):
    """body 0 of env i to xy[i], in the body state and in the env's last observation; returns the observed positions of
    body 0.  (An observation is taken by the env kernel at a reset or a step, not by set_body_state or observe(): the
    observed position is written into a snapshot of the env blocks at rv_get_state_ptrs' offset and loaded back.)"""
    t = world.torch
    st = world.body_state().clone()
    st[:, 0, 0:2] = t.as_tensor(np.asarray(xy, F), device=world.device)
    st[:, 0, 7:13] = 0.0
    world.set_body_state(st)
    view = abi.rv_state_view()
    lib.check(world.lib.rv_get_state_ptrs(world.h, C.byref(view)))
    snap = world.save_state()
    assert int(view.env_stride_bytes) == int(snap.blocks.shape[1])
    off = int(view.off_obs_pos)
    snap.blocks[:, off:off + 8] = t.as_tensor(np.asarray(xy, F).view(np.uint8).reshape(world.n, 8), device=world.device)
    world.load_state(snap)
    return _np(world.observe()['position'])[:, 0, :2]


@pytest.fixture(scope='module')
def world():
    w = _world(N, OFFSET)
    w.reset()
    yield w
    w.close()


def _placements(cfg):
    """body 0 onto the goal cell (D = 0), exactly midway between the centres of (2, 3) and (2, 4) (the tie), and where no
    cell is walkable: over (3, 5)"""
    r = host.Route(cfg)
    goal = int(np.flatnonzero(r.d == 0)[0])
    a, b = 2 * 8 + 3, 2 * 8 + 4
    return r, [(r.cx[goal] + F(0.02), r.cy[goal] - F(0.01)), (r.cx[a], F(0.5) * (r.cy[a] + r.cy[b])), (r.cx[3 * 8 + 5] - F(0.01), r.cy[3 * 8 + 5])]


@pytest.mark.parametrize('placed', [False, True], ids=['as_reset', 'placed'])
def test_kernel_equals_the_host_restatement(world, placed):
    world.reset(); world.observe()
    if placed:
        r, xy = _placements(world.cfg)
        p0 = _place(world, xy)
        assert _same(p0, np.asarray(xy, F))
        a, b = 2 * 8 + 3, 2 * 8 + 4
        qa = (r.cx[a] - p0[1, 0]) ** 2 + (r.cy[a] - p0[1, 1]) ** 2
        qb = (r.cx[b] - p0[1, 0]) ** 2 + (r.cy[b] - p0[1, 1]) ** 2
        assert qa == qb and r.aim(*p0[1]) == (a, 2 * 8 + 2)                  # the tie: the lower index
        assert r.aim(*p0[0])[0] == r.aim(*p0[0])[1] and r.d[r.aim(*p0[0])[0]] == 0      # on the goal cell
        assert not r.walk[3 * 8 + 5] and r.aim(*p0[2]) == (2 * 8 + 5, 2 * 8 + 4)        # off the tiles
    found = exhausted = 0
    for max_attempts in (1, 64, 130):
        for keep_nominal in (0, 1):
            for start_margin in (0.05, 0.3):
                kw = dict(plan_index=7, step=2, seed=0xfedcba98, max_attempts=max_attempts, keep_nominal=keep_nominal, start_margin=start_margin)
                a, st = _got(world, S, **kw)
                wa, wst = _want(world, S, offset=OFFSET, **kw)
                assert _same(st, wst) and _same(a, wa), kw
                found += int((st == abi.RV_HP_FOUND).sum()); exhausted += int((st == abi.RV_HP_EXHAUSTED).sum())
    assert found > 0 and exhausted > 0      # both ways out of the attempt loop were taken
    # a margin between the back-offs: a partial last round decides (attempts 128 and 129 of 130 belong to lanes 0 and 1)
    kw = dict(max_attempts=130, keep_nominal=0, start_margin=0.155, back_lo=0.08, back_hi=0.16)
    a, st = _got(world, S, **kw)
    wa, wst = _want(world, S, offset=OFFSET, **kw)
    assert _same(st, wst) and _same(a, wa)


def test_the_insertion_task_and_a_world_without_body_0():
    w = _world(N, OFFSET, task='insertion', layout=2)
    try:
        w.reset()
        kw = dict(plan_index=1, seed=4, max_attempts=64)
        a, st = _got(w, S, **kw)
        wa, wst = _want(w, S, offset=OFFSET, **kw)
        assert _same(st, wst) and _same(a, wa)
        # body 0 of env 1 switched off: no movable target -- the zero action, exhausted
        bp = w.body_params().clone()
        bp[1, 0, 0] = 0.0
        w.set_body_params(bp)
        pos, nb, mov = host.world_inputs(w.observe())
        assert mov.tolist() == [True, False, True]
        a, st = _got(w, S, **kw)
        wa, wst = _want(w, S, offset=OFFSET, **kw)
        assert _same(st, wst) and _same(a, wa)
        assert not a[1].any() and np.all(st[1] == abi.RV_HP_EXHAUSTED) and a[0].any()
    finally:
        w.close()


def test_candidates_of_the_source_are_one_candidate_of_each_branch(world):
    world.reset(); world.observe()
    plan = _world(N * S, OFFSET * S)
    try:
        plan.branch_from(world, S)
        kw = dict(plan_index=5, step=3, seed=2, max_attempts=64)
        a, st = _got(world, S, **kw)
        b, stb = _got(plan, 1, copies=S, **kw)
        assert _same(a, b.reshape(a.shape)) and _same(st, stb.reshape(st.shape))
        assert len({tuple(r) for r in a[0].reshape(S, -1).tolist()}) == S      # S different pushes
    finally:
        plan.close()


def test_plan_propose_route_equals_the_loop_of_separate_calls():
    n, s, h = 2, 3, 2
    src, plan = _world(n), _world(n * s)
    try:
        src.reset()
        before = _np(src.save_state().blocks)
        kw = dict(plan_index=6, seed=12, max_attempts=64)
        a, st, r, d, status = plan.plan_propose_route(src, lib.push_route_params(**kw), s, h)
        assert tuple(a.shape) == (n, s, h, src.G, 4) and tuple(status.shape) == (n, s, h)
        a, st, r, d, status = _np(a), _np(st), _np(r), _np(d), _np(status)
        assert _same(_np(src.save_state().blocks), before)      # the source is only read
        plan.branch_from(src, s)
        for t in range(h):
            at, stt = _got(plan, 1, copies=s, step=t, **kw)
            wat, wstt = _want(plan, 1, copies=s, step=t, **kw)
            assert _same(at, wat) and _same(stt, wstt)
            assert _same(a[:, :, t], at.reshape(n, s, src.G, 4)) and _same(status[:, :, t], stt.reshape(n, s)), t
            plan.set_actions(at[:, 0]); plan.step_macro()
            rew, done = plan.reward()
            assert _same(st[:, :, t], _np(plan.observe()['position'])[..., :2].reshape(n, s, abi.RV_MAXB, 2)), t
            assert _same(r[:, :, t], _np(rew).reshape(n, s)) and _same(d[:, :, t], _np(done).reshape(n, s)), t
        assert np.any(a[:, :, 1] != a[:, :, 0])
    finally:
        src.close(); plan.close()


def test_policy_equals_the_stated_loop():
    from robovat_amd import policies
    from robovat_amd.envs.push.push_env import VecPushEnv, PushEnv
    n, s, h, gamma = 3, 4, 2, 0.9
    cfg = configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0)
    env = VecPushEnv(n, config=cfg, seed=5)
    one = PushEnv(config=cfg, seed=5)
    try:
        env.reset(); one.reset()
        before = _np(env.save_state().blocks)
        kw = dict(seed=11, max_attempts=64, angle_jitter=0.2)
        policy = policies.RouteShootingPushPolicy(env, s, h, gamma=gamma, **kw)
        actions, best = policy.plan(env.get_observation())
        assert _same(_np(env.save_state().blocks), before)      # planning does not change the real env
        cand, states, rewards, dones, found = env.propose_route_plans(s, h, **kw)
        assert tuple(cand.shape) == (n, s, h) + tuple(env.action_shape) and tuple(found.shape) == (n, s, h)
        returns, _, want_best = env.score_plans(states, None, False, gamma)
        assert _same(_np(best), _np(want_best)) and _same(_np(policy.last_returns), _np(returns))
        assert _same(_np(policy.last_found), _np(found)) and policy.last_best is best
        assert _same(_np(actions), _np(cand)[np.arange(n), _np(want_best), 0])
        # the candidates of step 0 are the env's own route candidates; candidate 0 is the nominal push
        c0, f0 = env.sample_route_candidates(s, **kw)
        assert _same(_np(c0), _np(cand)[:, :, 0]) and _same(_np(f0), _np(found)[:, :, 0])
        nominal, _ = env.sample_route_candidates(1, seed=99)
        assert _same(_np(nominal)[:, 0], _np(c0)[:, 0])
        # no step in between: the same plan again
        again, _ = policy.plan()
        assert _same(_np(again), _np(actions))
        # one env: env 0 of the batch
        single = policies.RouteShootingPushPolicy(one, s, h, gamma=gamma, **kw)
        a1, b1 = single.plan()
        assert isinstance(a1, np.ndarray) and isinstance(b1, int) and _same(a1, _np(actions)[0]) and b1 == int(best[0])
        assert tuple(np.shape(one.propose_route_plans(s, h, **kw)[0])) == (s, h) + tuple(env.action_shape)
        assert tuple(np.shape(one.sample_route_candidates(s, **kw)[0])) == (s,) + tuple(env.action_shape)
        # ranking by the rewards the env gave
        by_reward = policies.RouteShootingPushPolicy(env, s, h, gamma=gamma, use_plan_reward=False, **kw)
        a2, b2 = by_reward.plan()
        assert np.array_equal(_np(b2), np.argmax(_np(by_reward.last_returns), axis=1))
        assert _same(_np(a2), _np(cand)[np.arange(n), _np(b2), 0])
        # after an env step the plan index has moved: other drawn candidates from the same state
        snap = env.save_state()
        env.step(actions)
        env.world.load_state(snap)      # (the state of before, the plan index of after)
        env.world.observe()
        other, _ = env.sample_route_candidates(s, **kw)
        assert _same(_np(other)[:, 0], _np(c0)[:, 0]) and not _same(_np(other)[:, 1:], _np(c0)[:, 1:])
        with pytest.raises(TypeError):
            env.sample_route_candidates(s, copies=2)
        with pytest.raises(TypeError):
            env.sample_route_candidates(s, no_such_field=1)
    finally:
        env.close(); one.close()


def test_refusals_leave_the_buffers_untouched(world):
    world.reset(); world.observe()
    t = world.torch
    s, h = 4, 2
    n = 2
    src = _world(n)
    plan, shifted, odd = _world(n * s), _world(n * s, offset=s), _world(n, offset=1)

    def no_goal(cfg): cfg.n_goal = 0
    def half_tile(cfg): cfg.region[1][0] = 1.5
    def far_tile(cfg): cfg.goal[0][1] = 8.0
    def neg_tile(cfg): cfg.region[0][1] = -1.0
    def nan_tile(cfg): cfg.goal[0][0] = float('nan')
    def clearing_task(cfg): cfg.task = abi.RV_TASK_CLEARING
    def no_task(cfg): cfg.task = abi.RV_TASK_NONE
    broken = [_world(n, edit=e) for e in (no_goal, half_tile, far_tile, neg_tile, nan_tile, clearing_task, no_task)]

    def buf(shape, value, dtype=None):
        return t.full(shape, value, dtype=dtype or t.float32, device=world.device)
    act, status = buf((n * s * h * world.G * 4 + 1,), 7.0), buf((n * s * h + 1,), -5, t.int32)
    states, rewards, dones = buf((n * s * h * abi.RV_MAXB * 2 + 1,), 3.0), buf((n * s * h,), 2.0), buf((n * s * h,), 9, t.uint8)
    field = buf((65,), 77, t.uint8)

    def ptr(x, off=0):
        return None if x is None else C.c_void_p(x.data_ptr() + off)

    def untouched():
        t.cuda.synchronize()
        return all(bool((x == v).all()) for x, v in ((act, 7.0), (status, -5), (states, 3.0), (rewards, 2.0), (dones, 9), (field, 77)))

    P = lib.push_route_params

    def multi(p=None, s_=s, w=src, a=act, st=status, null_params=False, off=0, st_off=0):
        p = p or P()
        return w.lib.rv_policy_route_multi(w.h, None if null_params else C.byref(p), s_, ptr(a, off), ptr(st, st_off))

    def propose(p=None, s_=s, h_=h, pl=plan, sr=src, a=act, null_params=False, off=0, st_off=0):
        p = p or P()
        return pl.lib.rv_plan_propose_route(pl.h, sr.h, None if null_params else C.byref(p), s_, h_, ptr(a, off), ptr(states, st_off),
                                            ptr(rewards), ptr(dones), ptr(status))

    def get_field(w, out=field):
        return w.lib.rv_get_route_field(w.h, ptr(out))
    env_cfg = configs.grasp_env_config()
    gscene, gnames = scenes.make_scene(env_cfg=env_cfg)
    gw = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=n, shape_names=gnames), gscene, device=0)
    try:
        bad_params = [P(max_attempts=0), P(max_attempts=abi.RV_HP_MAX_ATTEMPTS + 1), P(plan_index=-1), P(plan_index=1 << 24),
                      P(step=-1), P(step=64), P(copies=0), P(start_margin=-0.01), P(start_margin=np.nan),
                      P(angle_jitter=-0.01), P(angle_jitter=np.nan), P(lateral=-0.01), P(lateral=np.nan),
                      P(back_lo=0.2, back_hi=0.1), P(back_lo=np.nan), P(back_hi=np.nan),
                      P(length_lo=1.3, length_hi=1.2), P(length_lo=-0.1), P(length_lo=np.nan), P(length_hi=np.nan)]
        bad = [multi(p) for p in bad_params] + [propose(p) for p in bad_params]
        bad += [multi(s_=0), multi(s_=abi.RV_HP_MAX_SAMPLES + 1), multi(P(copies=257), s_=4), multi(null_params=True),
                multi(a=None), multi(off=2), multi(st_off=2), multi(w=gw),
                multi(P(copies=2), w=odd)]      # env_id_offset 1 is no multiple of 2 copies
        bad += [multi(w=w) for w in broken] + [get_field(w) for w in broken] + [get_field(gw), get_field(src, None)]
        bad += [propose(s_=0), propose(h_=0), propose(null_params=True), propose(a=None), propose(off=2), propose(st_off=4),
                propose(P(step=63)),               # step + h > 64
                propose(P(copies=257)),            # copies * s > RV_HP_MAX_SAMPLES
                propose(pl=shifted),               # env_id_offset is not s x the source's
                propose(pl=src), propose(s_=s + 1), propose(pl=gw, sr=gw)]
        assert bad == [abi.RV_ERR_VALUE] * len(bad)
        assert untouched()
        for call in (lambda: src.policy_route_multi(P(), 0), lambda: plan.plan_propose_route(src, P(), s, 0),
                     lambda: gw.policy_route_multi(P(), 2), lambda: gw.route_field(), lambda: broken[0].route_field()):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(TypeError):
            P(no_such_field=1)
        # the ends of the ranges are accepted
        src.reset()
        assert multi(P(plan_index=(1 << 24) - 1, step=63, max_attempts=abi.RV_HP_MAX_ATTEMPTS, start_margin=0.5)) == abi.RV_OK
        assert multi(P(copies=256, max_attempts=64, start_margin=0.0, angle_jitter=0.0, lateral=0.0, back_lo=0.1, back_hi=0.1,
                       length_lo=0.0, length_hi=0.0), s_=4, st=None) == abi.RV_OK
        assert propose(P(step=62, max_attempts=64)) == abi.RV_OK
        assert get_field(src) == abi.RV_OK
        t.cuda.synchronize()
        assert not untouched() and float(act[-1]) == 7.0 and int(status[-1]) == -5 and float(states[-1]) == 3.0 and int(field[-1]) == 77
        assert bool((field[:64] != 77).any())
    finally:
        for w in [src, plan, shifted, odd, gw] + broken:
            w.close()
