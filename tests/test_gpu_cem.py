"""rv_cem_sample / rv_cem_refit and CEMPushPolicy on the MI355X.  The kernels are compared bit for bit with
tests/cem_host.py (the float32 NumPy restatement of csrc/rv_dev_cem.h) on synthetic distributions and returns; the policy
with a loop the test drives itself: cem_host samples and refits on the CPU, the env simulates and scores, plan_host
ranks."""
import ctypes as C

import numpy as np
import pytest

import cem_host as host
import plan_host
from robovat_amd import abi, configs, lib, scenes

pytestmark = pytest.mark.gpu
F = np.float32
N, SEED = 3, 7 + (5 << 32)
NAN, INF = np.nan, np.inf
H_MAX = abi.RV_CEM_MAX_DIM // 4      # the longest horizon without goal steps: D = RV_CEM_MAX_DIM


def _horizons(s):
    """1, 3, 17 for every S; the longest one (a thread of the smallest workgroup then owns eight floats of the plan) at one
    S per workgroup shape"""
    return (1, 3, 17) + ((H_MAX,) if s in (5, 200, 1024) else ())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _world(n, offset=0, seed=SEED):
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n,
                                 shape_names=names, env_id_offset=offset, seed=seed)
    return lib.World(cfg, scene, device=0)


@pytest.fixture(scope='module')
def world():
    w = _world(N)
    yield w
    w.close()


def _dist(n, d, seed):
    rng = np.random.RandomState(seed)
    mean, std = rng.uniform(-0.9, 0.9, (n, d)).astype(F), rng.uniform(0.0, 0.8, (n, d)).astype(F)
    mean[0, :4] = [1.0, -1.0, 1.5, -1.5]      # on and beyond the bounds
    std[0, 0] = std[0, 1] = 1.0
    std[n - 1, ::2] = 0.0                     # no spread: clamp(mean)
    return mean, std


def _returns(n, s, seed):
    """ties, both zeros, infinities and NaNs among the returns; one env all equal"""
    rng = np.random.RandomState(seed)
    r = np.round(rng.standard_normal((n, s)) * 2.0).astype(F)      # (rounded: many ties)
    special = np.array([NAN, INF, -INF, -0.0, 0.0, NAN, INF], F)
    k = min(s, len(special))
    r[0, rng.permutation(s)[:k]] = special[:k]
    r[1, :] = F(2.5)
    return r


@pytest.mark.parametrize('s', [1, 5, 64, 65, 200, 1024])
def test_sample_equals_the_host_restatement(world, s):
    for h in _horizons(s):
        d = h * world.G * 4
        mean, std = _dist(N, d, seed=s + h)
        for keep in (True, False):
            p = lib.cem_params(plan_index=11, iteration=2, seed=0xfedcba98, keep_mean=int(keep))
            got = world.cem_sample(mean, std, p, s, h)
            assert tuple(got.shape) == (N, s, h, world.G, 4)
            want = host.cem_sample(mean, std, s, world_seed=SEED, plan_index=11, iteration=2, seed=0xfedcba98, keep_mean=keep)
            assert _same(got.cpu().numpy().reshape(N, s, d), want), (s, h, keep)
    # a buffer that is only 4-byte aligned takes the scalar stores: the same values
    t = world.torch
    m, sd = t.as_tensor(mean, device=world.device), t.as_tensor(std, device=world.device)
    buf = t.zeros(N * s * d + 1, dtype=t.float32, device=world.device)
    assert buf[1:].data_ptr() % 16 != 0
    lib.check(world.lib.rv_cem_sample(world.h, C.byref(p), C.c_void_p(m.data_ptr()), C.c_void_p(sd.data_ptr()), s, h, C.c_void_p(buf[1:].data_ptr())))
    assert _same(buf[1:].cpu().numpy().reshape(N, s, d), want) and float(buf[0]) == 0.0


@pytest.mark.parametrize('s', [1, 5, 64, 65, 200, 1024])
def test_refit_equals_the_host_restatement(world, s):
    for h in _horizons(s):
        d = h * world.G * 4
        mean, std = _dist(N, d, seed=2 * s + h)
        x = host.cem_sample(mean, std, s, world_seed=SEED, iteration=1, keep_mean=True)
        returns = _returns(N, s, seed=s + 3 * h)
        for e, alpha, floor, with_elite in {(1, 0.0, 0.0, True), (s, 0.5, 0.0, False), (max(1, s // 8), 0.0, 0.05, True),
                                            (max(1, s // 3), 0.3, 0.4, True)}:
            p = lib.cem_params(n_elites=e, alpha=alpha, min_std=floor)
            m, sd, el = world.cem_refit(x.reshape(N, s, h, world.G, 4), returns, mean, std, p, elite=with_elite)
            hm, hs, hel = host.cem_refit(x, returns, mean, std, e, alpha, floor)
            assert _same(m.cpu().numpy(), hm) and _same(sd.cpu().numpy(), hs), (s, h, e, alpha, floor)
            assert (el is None) if not with_elite else _same(el.cpu().numpy(), hel)
            assert np.all(hs >= F(floor))
    assert hel[1].tolist() == list(range(len(hel[1])))      # all returns equal: the elites are 0 .. E-1


def test_ranking_of_special_returns(world):
    r = np.zeros((N, 10), F)
    r[0] = [0.0, NAN, -INF, 3.0, -0.0, INF, 3.0, NAN, -1.0, 0.0]
    r[2] = NAN
    x = np.random.RandomState(1).uniform(-1, 1, (N, 10, 4)).astype(F)
    mean, std = np.zeros((N, 4), F), np.ones((N, 4), F)
    _, _, el = world.cem_refit(x.reshape(N, 10, 1, world.G, 4), r, mean, std, lib.cem_params(n_elites=10))
    el = el.cpu().numpy()
    assert el[0].tolist() == [5, 3, 6, 0, 4, 9, 8, 2, 1, 7]
    assert el[1].tolist() == list(range(10)) and el[2].tolist() == list(range(10))
    assert _same(el, host.cem_refit(x, r, mean, std, 10)[2])


def test_a_shard_draws_what_the_whole_world_draws():
    whole, shard = _world(4), _world(2, offset=2)
    try:
        mean, std = _dist(4, 12, seed=9)
        p = lib.cem_params(plan_index=5, iteration=1, seed=3, keep_mean=0)
        a = whole.cem_sample(mean, std, p, 65, 3).cpu().numpy()
        b = shard.cem_sample(mean[2:], std[2:], p, 65, 3).cpu().numpy()
        assert _same(a[2:], b) and not _same(a[:2], b)
    finally:
        whole.close(); shard.close()


def test_refusals_leave_the_buffers_untouched(world):
    t = world.torch
    s, h = 8, 2
    d = h * world.G * 4

    def buf(shape, value, dtype=None):
        return t.full(shape, value, dtype=dtype or t.float32, device=world.device)
    mean, std, act, ret = buf((N, d), 0.25), buf((N, d), 0.5), buf((N, s, d), 7.0), buf((N, s), 1.0)
    elite = buf((N, s), -5, t.int32)

    def ptr(x):
        return None if x is None else C.c_void_p(x.data_ptr())

    def untouched():
        t.cuda.synchronize()
        return (bool((mean == 0.25).all()) and bool((std == 0.5).all()) and bool((act == 7.0).all()) and bool((elite == -5).all()))

    def sample(p=None, s_=s, h_=h, m=mean, sd=std, a=act, null_params=False):
        p = p or lib.cem_params()
        return world.lib.rv_cem_sample(world.h, None if null_params else C.byref(p), ptr(m), ptr(sd), s_, h_, ptr(a))

    def refit(p=None, s_=s, h_=h, a=act, r=ret, m=mean, sd=std, null_params=False):
        p = p or lib.cem_params(n_elites=2)
        return world.lib.rv_cem_refit(world.h, None if null_params else C.byref(p), ptr(a), ptr(r), s_, h_, ptr(m), ptr(sd), ptr(elite))
    too_long = abi.RV_CEM_MAX_DIM // (world.G * 4) + 1
    bad = [sample(s_=0), sample(s_=abi.RV_CEM_MAX_SAMPLES + 1), sample(h_=0), sample(h_=too_long), sample(null_params=True),
           sample(m=None), sample(sd=None), sample(a=None),
           sample(lib.cem_params(plan_index=-1)), sample(lib.cem_params(plan_index=1 << 24)),
           sample(lib.cem_params(iteration=-1)), sample(lib.cem_params(iteration=1 << 15)),
           refit(s_=0), refit(s_=abi.RV_CEM_MAX_SAMPLES + 1), refit(h_=0), refit(h_=too_long), refit(null_params=True),
           refit(a=None), refit(r=None), refit(m=None), refit(sd=None),
           refit(lib.cem_params(n_elites=0)), refit(lib.cem_params(n_elites=s + 1)),
           refit(lib.cem_params(n_elites=2, alpha=-0.1)), refit(lib.cem_params(n_elites=2, alpha=1.0)),
           refit(lib.cem_params(n_elites=2, alpha=NAN)), refit(lib.cem_params(n_elites=2, min_std=-1e-3)),
           refit(lib.cem_params(n_elites=2, min_std=NAN)),
           refit(lib.cem_params(n_elites=2, plan_index=1 << 24)), refit(lib.cem_params(n_elites=2, iteration=1 << 15))]
    assert bad == [abi.RV_ERR_VALUE] * len(bad)
    assert untouched()
    with pytest.raises(ValueError):
        world.cem_sample(mean, std, lib.cem_params(), 0, h)
    with pytest.raises(ValueError):
        world.cem_sample(mean, std, lib.cem_params(), s, h + 1)      # mean / std of another horizon
    with pytest.raises(TypeError):
        lib.cem_params(no_such_field=1)
    # the largest plan index, iteration, sample count and dimension are accepted
    assert sample(lib.cem_params(plan_index=(1 << 24) - 1, iteration=(1 << 15) - 1)) == abi.RV_OK
    assert refit(lib.cem_params(n_elites=s, alpha=0.0, min_std=0.0)) == abi.RV_OK
    t.cuda.synchronize()
    assert not untouched()
    # a grasp world has no push plans
    env_cfg = configs.grasp_env_config()
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    gw = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=N, shape_names=names), scene, device=0)
    try:
        g = gw.G * 4
        with pytest.raises(ValueError):
            gw.cem_sample(np.zeros((N, g), F), np.ones((N, g), F), lib.cem_params(), 4, 1)
        with pytest.raises(ValueError):
            gw.cem_refit(np.zeros((N, 4, 1, gw.G, 4), F), np.zeros((N, 4), F), np.zeros((N, g), F), np.ones((N, g), F), lib.cem_params())
    finally:
        gw.close()


# ---- the policy: N = 3, S = 8, H = 2, I = 2, E = 3 on crossing layout 0 (the shapes of test_gpu_shooting_policy.py)
S, H, ITERS, ELITES, GAMMA, ENV_SEED = 8, 2, 2, 3, 0.9, 5
KW = dict(num_iterations=ITERS, num_elites=ELITES, gamma=GAMMA, init_std=0.5, min_std=0.05, alpha=0.25)


@pytest.fixture(scope='module')
def env():
    from robovat_amd.envs.push.push_env import VecPushEnv
    e = VecPushEnv(N, config=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), seed=ENV_SEED)
    e.reset()
    yield e
    e.close()


def _drive(env, seed, mean0):
    """the planner's loop with cem_host on the CPU; simulation and scoring by the env, the ranking by plan_host"""
    t = env.world.torch
    a = int(np.prod(env.action_shape))
    d = H * a
    state0 = env.get_observation()['position'][..., :2].cpu().numpy()
    tiles = plan_host.Tiles('crossing', 0)
    mean, std = np.ascontiguousarray(mean0, F).reshape(N, d), np.full((N, d), 0.5, F)
    all_ret, best = [], None
    for it in range(ITERS):
        cand = host.cem_sample(mean, std, S, world_seed=ENV_SEED, plan_index=env._macro_index, iteration=it, seed=seed, keep_mean=True)
        states, _, _ = env.simulate_plans(t.as_tensor(cand.reshape((N, S, H) + tuple(env.action_shape)), device=env.device))
        ret, _, idx = plan_host.plan_score(tiles, state0, states.cpu().numpy(), gamma=GAMMA)
        val = ret[np.arange(N), idx]
        act = cand.reshape(N, S, H, a)[np.arange(N), idx, 0]
        if best is None:
            best = [val.copy(), np.zeros(N, np.int32), idx.astype(np.int32), act.copy()]
        else:
            better = val > best[0]
            best[0][better], best[1][better], best[2][better], best[3][better] = val[better], it, idx[better], act[better]
        all_ret.append(ret)
        mean, std, _ = host.cem_refit(cand, ret, mean, std, ELITES, KW['alpha'], KW['min_std'])
    shape = (N, H) + tuple(env.action_shape)
    return best[3].reshape((N,) + tuple(env.action_shape)), mean.reshape(shape), std.reshape(shape), np.stack(all_ret), best[1], best[2]


def _check(policy, out, want):
    actions, (b_it, b_idx) = out
    w_act, w_mean, w_std, w_ret, w_it, w_idx = want
    assert _same(actions.cpu().numpy(), w_act)
    assert _same(policy.last_mean.cpu().numpy(), w_mean) and _same(policy.last_std.cpu().numpy(), w_std)
    assert _same(policy.last_returns.cpu().numpy(), w_ret)
    assert _same(b_it.cpu().numpy(), w_it) and _same(b_idx.cpu().numpy(), w_idx)
    assert policy.last_best[0] is b_it and policy.last_best[1] is b_idx


def test_policy_equals_the_host_driven_loop_and_leaves_the_env_alone(env):
    from robovat_amd import policies
    before = env.save_state().blocks.cpu().numpy()
    policy = policies.CEMPushPolicy(env, S, H, seed=11, **KW)
    zeros = np.zeros((N, H) + tuple(env.action_shape), F)
    assert _same(policy.initial_mean().cpu().numpy(), zeros)
    out = policy.plan(env.get_observation())
    assert _same(env.save_state().blocks.cpu().numpy(), before)      # planning does not change the real env
    _check(policy, out, _drive(env, 11, zeros))
    assert tuple(out[0].shape) == (N,) + tuple(env.action_shape) and tuple(policy.last_returns.shape) == (ITERS, N, S)
    # warm start: the next call begins at this call's final mean, one step on, zeros in the last step
    final = policy.last_mean.cpu().numpy()
    shifted = np.concatenate([final[:, 1:], np.zeros_like(final[:, :1])], axis=1)
    assert _same(policy.initial_mean().cpu().numpy(), shifted)
    out2 = policy.plan()
    _check(policy, out2, _drive(env, 11, shifted))
    # reset(mask) forgets the warm start of the masked envs only
    again = policy.initial_mean().cpu().numpy()
    policy.reset(np.array([True, False, False]))
    cleared = policy.initial_mean().cpu().numpy()
    assert _same(cleared[0], np.zeros_like(cleared[0])) and _same(cleared[1:], again[1:]) and np.any(again[0] != 0)
    policy.reset()
    assert _same(policy.initial_mean().cpu().numpy(), zeros)
    assert tuple(policy.action(None).shape) == (N,) + tuple(env.action_shape)
    assert _same(env.save_state().blocks.cpu().numpy(), before)
    cold = policies.CEMPushPolicy(env, S, H, seed=11, warm_start=False, **KW)
    first = cold.plan()
    _check(cold, cold.plan(), _drive(env, 11, zeros))      # without warm start every call begins at zero
    assert _same(first[0].cpu().numpy(), cold.plan()[0].cpu().numpy())
    assert policies.CEMPushPolicy(env, 64, H).num_elites == 8 and policies.CEMPushPolicy(env, 5, H).num_elites == 1


def test_same_seed_from_the_same_restored_snapshot_gives_the_same_plan(env):
    from robovat_amd import policies
    snap = env.save_state()
    first = policies.CEMPushPolicy(env, S, H, seed=3, **KW)
    a1, b1 = first.plan()
    env.step(a1)                                                  # the env moves on ...
    assert not _same(env.save_state().blocks.cpu().numpy(), snap.blocks.cpu().numpy())
    env.restore_state(snap)                                       # ... and comes back
    second = policies.CEMPushPolicy(env, S, H, seed=3, **KW)
    a2, b2 = second.plan()
    assert _same(a1.cpu().numpy(), a2.cpu().numpy()) and _same(b1[0].cpu().numpy(), b2[0].cpu().numpy()) and _same(b1[1].cpu().numpy(), b2[1].cpu().numpy())
    assert _same(first.last_mean.cpu().numpy(), second.last_mean.cpu().numpy()) and _same(first.last_returns.cpu().numpy(), second.last_returns.cpu().numpy())
    other = policies.CEMPushPolicy(env, S, H, seed=4, **KW)
    a3, _ = other.plan()
    assert not _same(a1.cpu().numpy(), a3.cpu().numpy()) and not _same(first.last_mean.cpu().numpy(), other.last_mean.cpu().numpy())


def test_ranking_by_the_recorded_env_rewards(env):
    from robovat_amd import policies
    policy = policies.CEMPushPolicy(env, S, H, seed=7, use_plan_reward=False, **KW)
    actions, (b_it, b_idx) = policy.plan()
    r = policy.last_returns.cpu().numpy()
    per_it = r.max(axis=2)                                        # [I, N]
    want_it = np.argmax(per_it, axis=0)                           # (the first of equal maxima: the lowest iteration)
    assert np.array_equal(b_it.cpu().numpy(), want_it)
    assert np.array_equal(b_idx.cpu().numpy(), np.argmax(r[want_it, np.arange(N)], axis=1))
    assert np.abs(actions.cpu().numpy()).max() <= 1.0


def test_one_env_gets_one_action():
    from robovat_amd import policies
    from robovat_amd.envs.push.push_env import PushEnv
    e = PushEnv(config=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), seed=ENV_SEED)
    try:
        e.reset()
        policy = policies.CEMPushPolicy(e, S, H, seed=2, **KW)
        action, (b_it, b_idx) = policy.plan()
        assert isinstance(action, np.ndarray) and action.shape == tuple(e.action_space.shape) and action.dtype == F
        assert isinstance(b_it, int) and isinstance(b_idx, int) and 0 <= b_it < ITERS and 0 <= b_idx < S
        assert e.action_space.contains(action)
        cand = e.sample_plan_candidates(np.zeros((H,) + action.shape, F), np.full((H,) + action.shape, 0.5, F), S, 0, seed=2)
        assert tuple(cand.shape) == (S, H) + action.shape
        m, sd, el = e.refit_plan_distribution(cand, np.arange(S, dtype=F), np.zeros((H,) + action.shape, F), np.ones((H,) + action.shape, F), 2)
        assert tuple(m.shape) == (H,) + action.shape and tuple(sd.shape) == tuple(m.shape) and el.cpu().numpy().tolist() == [S - 1, S - 2]
        assert policy.action(None).shape == action.shape
    finally:
        e.close()
