"""ShootingPushPolicy on the MI355X: random-shooting MPC over VecPushEnv.simulate_plans, ranked by the planning-mode
PushReward.  The ranking is checked against tests/plan_host.py applied on the CPU to the states the simulator returned;
planning is repeatable from a restored snapshot and leaves the real env alone.  (No success-rate bar: DESIGN.md 14.)"""
import numpy as np
import pytest

import plan_host as host
from robovat_amd import abi, configs

pytestmark = pytest.mark.gpu
N, S, H, SEED = 3, 8, 2, 5
GAMMA = 0.9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope='module')
def env():
    from robovat_amd.envs.push.push_env import VecPushEnv
    e = VecPushEnv(N, config=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), seed=SEED)
    e.reset()
    yield e
    e.close()


def _candidates(env, seed):
    """the candidates the policy draws first from `seed`"""
    import torch
    g = torch.Generator(device=env.device)
    g.manual_seed(seed)
    shape = (N, S, H) + tuple(env.action_shape)
    return torch.rand(shape, generator=g, device=env.device, dtype=torch.float32) * 2.0 - 1.0


def test_best_plan_is_the_arg_max_of_the_host_score_and_the_env_is_untouched(env):
    from robovat_amd import policies
    snap = env.save_state()
    before = snap.blocks.cpu().numpy()
    state0 = env.get_observation()['position'][..., :2].cpu().numpy()
    policy = policies.ShootingPushPolicy(env, num_samples=S, horizon=H, gamma=GAMMA, seed=11)
    actions, best = policy.plan(env.get_observation())
    assert _same(env.save_state().blocks.cpu().numpy(), before)      # planning does not change the real env
    cand = _candidates(env, 11)
    states, _, _ = env.simulate_plans(cand)
    T = host.Tiles('crossing', 0)
    h_ret, _, h_best = host.plan_score(T, state0, states.cpu().numpy(), gamma=GAMMA)
    assert best.dtype == env.world.torch.int32 and _same(best.cpu().numpy(), h_best)
    assert _same(policy.last_returns.cpu().numpy(), h_ret)
    assert _same(actions.cpu().numpy(), cand.cpu().numpy()[np.arange(N), h_best, 0])
    assert tuple(actions.shape) == (N,) + tuple(env.action_shape)
    assert tuple(policy.action(None).shape) == tuple(actions.shape)
    assert _same(env.save_state().blocks.cpu().numpy(), before)


def test_same_seed_from_the_same_restored_snapshot_gives_the_same_actions(env):
    from robovat_amd import policies
    snap = env.save_state()
    first = policies.ShootingPushPolicy(env, S, H, GAMMA, seed=3).plan()
    env.step(first[0])                                            # the env moves on ...
    assert not _same(env.save_state().blocks.cpu().numpy(), snap.blocks.cpu().numpy())
    env.restore_state(snap)                                       # ... and comes back
    second = policies.ShootingPushPolicy(env, S, H, GAMMA, seed=3).plan()
    assert _same(first[0].cpu().numpy(), second[0].cpu().numpy()) and _same(first[1].cpu().numpy(), second[1].cpu().numpy())
    other = policies.ShootingPushPolicy(env, S, H, GAMMA, seed=4).plan()
    assert not _same(first[0].cpu().numpy(), other[0].cpu().numpy())


def test_ranking_by_the_recorded_env_rewards(env):
    from robovat_amd import policies
    policy = policies.ShootingPushPolicy(env, S, H, GAMMA, seed=7, use_plan_reward=False)
    actions, best = policy.plan()
    cand = _candidates(env, 7)
    _, rewards, _ = env.simulate_plans(cand)
    r = rewards.cpu().numpy()
    want = (r * (np.float32(GAMMA) ** np.arange(H, dtype=np.float32))[None, None]).sum(axis=2, dtype=np.float32)
    assert np.array_equal(best.cpu().numpy(), np.argmax(policy.last_returns.cpu().numpy(), axis=1))
    assert np.allclose(policy.last_returns.cpu().numpy(), want, rtol=0, atol=4 * np.finfo(np.float32).eps * np.abs(r).sum(axis=2).max())
    assert _same(actions.cpu().numpy(), cand.cpu().numpy()[np.arange(N), best.cpu().numpy(), 0])
