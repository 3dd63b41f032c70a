"""The plumbing the look-ahead policies and the ``lib.*_params`` builders share, on stub envs and CPU torch: no library,
no GPU.  What the kernels compute is pinned by the GPU tests; here: the ranking expression bit for bit, the gather and
the single-env unwrap, "the lowest index that qualifies, else 0", the single-env refusal, and the override loop."""
import types

import numpy as np
import pytest
import torch

from robovat_amd import lib, policies

N, S, H, A = 2, 3, 2, (4,)


class PushVec(object):
    """a VecPushEnv as the push policies see it, with canned returns"""

    def __init__(self, n, cand, rewards, scored=None):
        self.world = types.SimpleNamespace(torch=torch)
        self.device, self.num_envs, self.action_shape = 'cpu', n, A
        self.cand, self.rewards, self.scored = cand, rewards, scored
        self.states = torch.zeros((n, S, H, 4, 2))
        self.dones = torch.zeros((n, S, H), dtype=torch.bool)
        self.found = torch.ones((n, S, H), dtype=torch.bool)
        self.calls = []

    def simulate_plans(self, cand):
        self.calls.append(('simulate_plans', cand))
        return self.states, self.rewards, self.dones

    def propose_plans(self, *args):
        self.calls.append(('propose_plans', args))
        return self.cand, self.states, self.rewards, self.dones, self.found

    def propose_route_plans(self, *args, **route):
        self.calls.append(('propose_route_plans', args, route))
        return self.cand, self.states, self.rewards, self.dones, self.found

    def score_plans(self, states, state, is_high_level, gamma):
        self.calls.append(('score_plans', states, state, is_high_level, gamma))
        return self.scored[0], None, self.scored[1]


def shooting_draw(n, seed):
    """the candidates ShootingPushPolicy draws from its generator: what the other two are handed as proposals"""
    gen = torch.Generator(device='cpu')
    gen.manual_seed(seed)
    return torch.rand((n, S, H) + A, generator=gen, device='cpu', dtype=torch.float32) * 2.0 - 1.0


def bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize('gamma', [1.0, 0.9])
def test_rank_is_the_expression_it_replaced(gamma):
    nan = float('nan')
    rewards = torch.tensor([[[0.25, -1.5], [0.75, 3.0], [0.75, 3.0]],      # candidates 1 and 2 tie for the maximum
                            [[1.0, 2.0], [nan, 0.5], [4.0, 8.0]]], dtype=torch.float32)
    v = PushVec(N, None, rewards)
    policy = policies.ShootingPushPolicy(v, S, H, gamma=gamma, use_plan_reward=False)
    returns, best = policy._rank(v.states, rewards)
    t = torch
    disc = t.full((H,), gamma, device='cpu', dtype=t.float32) ** t.arange(H, device='cpu')
    want = (rewards * disc).sum(dim=2)
    want_best = want.argmax(dim=1).to(t.int32)
    assert returns.dtype == t.float32 and best.dtype == t.int32
    assert t.equal(bits(returns), bits(want)) and t.equal(best, want_best)
    assert int(best[0]) == 1                           # the first of equal maxima
    assert bool(t.isnan(returns[1, 1])) and int(best[1]) == int(want.argmax(dim=1)[1])      # a NaN row: as argmax has it
    assert v.calls == []                               # nothing is scored on the device


def test_rank_with_the_plan_reward_is_score_plans():
    scored = (torch.tensor([[1.0, 5.0, 5.0], [0.0, -1.0, -2.0]]), torch.tensor([1, 0], dtype=torch.int32))
    v = PushVec(N, None, torch.zeros((N, S, H)), scored)
    policy = policies.CEMPushPolicy(v, S, H, gamma=0.9, is_high_level=True)
    returns, best = policy._rank(v.states, None)
    assert returns is scored[0] and best is scored[1]
    (name, states, state, high, gamma), = v.calls
    assert (name, state, high, gamma) == ('score_plans', None, True, 0.9) and states is v.states


def _three(env, vec, seed):
    return (policies.ShootingPushPolicy(env, S, H, gamma=0.9, seed=seed, use_plan_reward=False),
            policies.HeuristicShootingPushPolicy(env, S, H, gamma=0.9, seed=seed, use_plan_reward=False),
            policies.RouteShootingPushPolicy(env, S, H, gamma=0.9, seed=seed, use_plan_reward=False, max_attempts=7))


def test_the_three_shooting_policies_agree_on_the_same_candidates():
    cand = shooting_draw(N, 3)
    rewards = torch.tensor([[[0.0, 1.0], [2.0, 0.0], [0.5, 0.5]], [[1.0, 1.0], [0.0, 0.0], [1.0, 2.0]]])
    v = PushVec(N, cand, rewards)
    want_best = torch.tensor([1, 2], dtype=torch.int32)
    want_actions = torch.stack([cand[0, 1, 0], cand[1, 2, 0]])
    for policy in _three(v, v, 3):
        actions, best = policy.plan()
        assert torch.equal(best, want_best) and best.dtype == torch.int32
        assert torch.equal(bits(actions), bits(want_actions)) and tuple(actions.shape) == (N,) + A
        assert policy.last_best is best and tuple(policy.last_returns.shape) == (N, S)
    shooting, heuristic, route = _three(v, v, 3)
    assert not hasattr(shooting, 'last_found')
    heuristic.plan(); route.plan()
    assert heuristic.last_found is v.found and route.last_found is v.found
    # the candidate sources were asked as before
    assert v.calls[-2] == ('propose_plans', (S, H, 3, 20000, 0.05, 0.01))
    assert v.calls[-1] == ('propose_route_plans', (S, H, 3), {'max_attempts': 7})
    shooting.plan()
    assert v.calls[-1][0] == 'simulate_plans' and torch.equal(bits(v.calls[-1][1]), bits(cand))


def test_a_single_env_gets_a_numpy_action_and_an_int():
    cand = shooting_draw(1, 4)
    rewards = torch.tensor([[[0.0, 1.0], [0.0, 0.5], [3.0, 0.0]]])
    v = PushVec(1, cand, rewards)
    env = types.SimpleNamespace(_vec=v)      # (a PushEnv is a VecPushEnv of one)
    for policy in _three(env, v, 4):
        action, best = policy.plan()
        assert isinstance(action, np.ndarray) and action.shape == A and action.dtype == np.float32
        assert type(best) is int and best == 2
        assert np.array_equal(action, cand[0, 2, 0].numpy())
        assert torch.is_tensor(policy.last_best)      # (the kept tensors stay tensors)


@pytest.mark.parametrize('cls', ['ShootingPushPolicy', 'HeuristicShootingPushPolicy', 'RouteShootingPushPolicy'])
def test_the_refusal_names_the_class(cls):
    v = PushVec(N, None, None)
    with pytest.raises(ValueError) as e:
        getattr(policies, cls)(v, 0, H)
    assert str(e.value) == cls + ': num_samples and horizon must be positive'
    with pytest.raises(ValueError) as e:
        policies.CEMPushPolicy(v, S, H, num_iterations=0)
    assert str(e.value) == 'CEMPushPolicy: num_samples, horizon and num_iterations must be positive'


class GraspVec(object):
    """a VecGrasp4DofEnv as the grasp policies see it"""

    def __init__(self, n, k, status):
        self.world = types.SimpleNamespace(torch=torch, render=self._render)
        self.device, self.num_envs = 'cpu', n
        self.cand = torch.arange(n * k * 4, dtype=torch.float32).reshape(n, k, 4)
        self.antipodal_status = torch.tensor(status, dtype=torch.int32)
        self.antipodal_count = torch.full((n,), k, dtype=torch.int32)
        self.antipodal_actions4 = self.cand
        self.antipodal_image_grasps = torch.zeros((n, k, 5))
        self.rendered, self.sampled = 0, []

    def _render(self):
        self.rendered += 1
        return torch.ones((self.num_envs, 6, 8)), None

    def sample_antipodal_candidates(self, k, depth, config):
        self.sampled.append(depth)
        return self.cand

    def try_grasps(self, actions4):
        return self.rewards, None

    def grasp_qualities(self, model, grasps, depth, **crop):
        return self.logits

    def refine_grasps(self, *args, **kwargs):
        raise AssertionError('not reached')


def test_first_index():
    v = GraspVec(3, 4, [1, 1, 1])
    policy = policies.LookaheadGrasp4DofPolicy(v, 4)
    q = torch.tensor([[False, False, False, False], [False, False, False, True], [False, True, False, True]])
    first = policy._first_index(q)
    assert first.tolist() == [0, 3, 1] and first.dtype == torch.int64
    # through the policy: the lowest index with a positive reward, else candidate 0
    v.rewards = torch.tensor([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], [0.0, 2.0, 0.0, 1.0]])
    actions = policy.action(None)
    assert policy.last_choice.tolist() == [0, 3, 1]
    assert torch.equal(actions, torch.stack([v.cand[0, 0], v.cand[1, 3], v.cand[2, 1]]))
    # GraspQualityPolicy: the highest logit among the valid rows, the lower index among equals; a NaN best: candidate 0
    v.logits = torch.tensor([[1.0, 5.0, 5.0, 9.0], [0.0, float('nan'), 0.0, 0.0], [3.0, 2.0, 1.0, 0.0]])
    v.antipodal_count = torch.tensor([3, 4, 0], dtype=torch.int32)
    quality = policies.GraspQualityPolicy(v, object(), 4)
    quality.action(None)
    assert quality.last_choice.tolist() == [1, 0, 0]


def test_who_renders():
    """LookaheadGrasp4DofPolicy hands a missing depth on to the sampler; the other two render once themselves"""
    v = GraspVec(2, 3, [1, 1])
    v.rewards = torch.zeros((2, 3))
    v.logits = torch.zeros((2, 3))
    policies.LookaheadGrasp4DofPolicy(v, 3).action(None)
    assert v.rendered == 0 and v.sampled == [None]
    policies.LookaheadGrasp4DofPolicy(v, 3).action({})
    assert v.rendered == 0 and v.sampled == [None, None]
    policies.GraspQualityPolicy(v, object(), 3).action(None)
    assert v.rendered == 1 and tuple(v.sampled[-1].shape) == (2, 6, 8)
    depth = torch.zeros((2, 6, 8))
    policies.GraspQualityPolicy(v, object(), 3).action({'depth': depth})
    assert v.rendered == 1 and v.sampled[-1] is depth


@pytest.mark.parametrize('status', [0, 2, -1])
def test_a_single_env_without_a_grasp_is_refused(status):
    v = GraspVec(1, 3, [status])
    env = types.SimpleNamespace(_vec=v)      # (a Grasp4DofEnv is a VecGrasp4DofEnv of one)
    depth = np.zeros((6, 8), np.float64)
    made = (policies.LookaheadGrasp4DofPolicy(env, 3), policies.GraspQualityPolicy(env, object(), 3),
            policies.CEMGraspPolicy(env, 3, model=object()))
    for policy in made:
        with pytest.raises(ValueError) as e:
            policy.action({'depth': depth})
        assert str(e.value) == 'Failed to sample any valid grasp (antipodal status %d).' % status
        # the single env's depth went to the sampler as float32 [1, H, W]
        assert v.sampled[-1].shape == (1, 6, 8) and v.sampled[-1].dtype == np.float32
    assert v.rendered == 0
    # a batched env is not refused: its rows without a grasp fall back to candidate 0
    v.rewards = torch.zeros((1, 3))
    assert tuple(policies.LookaheadGrasp4DofPolicy(v, 3).action(None).shape) == (1, 4)


def test_a_single_env_with_a_grasp_gets_numpy():
    v = GraspVec(1, 3, [1])
    v.rewards = torch.tensor([[0.0, 1.0, 1.0]])
    policy = policies.LookaheadGrasp4DofPolicy(types.SimpleNamespace(_vec=v), 3)
    action = policy.action({'depth': np.zeros((6, 8), np.float64)})
    assert isinstance(action, np.ndarray) and np.array_equal(action, v.cand[0, 1].numpy())
    assert policy.last_choice == 1 and type(policy.last_choice) is int and isinstance(policy.last_rewards, np.ndarray)
    assert v.sampled[-1].shape == (1, 6, 8) and v.sampled[-1].dtype == np.float32


@pytest.mark.parametrize('cls,args', [('LookaheadGrasp4DofPolicy', (3,)), ('GraspQualityPolicy', (object(), 3)),
                                      ('CEMGraspPolicy', (3,))])
def test_an_env_without_the_method_is_refused_by_name(cls, args):
    with pytest.raises(NotImplementedError) as e:
        getattr(policies, cls)(types.SimpleNamespace(), *args)
    assert str(e.value) == cls + ' needs a Grasp4DofEnv / VecGrasp4DofEnv'


# builder, a field of an integer type, whether the struct has reserved words
BUILDERS = [('plan_params', 'n_bodies', False), ('cem_params', 'n_elites', False), ('push_proposal_params', 'max_attempts', False),
            ('push_route_params', 'max_attempts', False), ('depth_noise_params', 'rescale_factor', False),
            ('grasp_crop_params', 'height', True), ('grasp_refine_params', 'height', True)]


@pytest.mark.parametrize('name,int_field,has_reserved', BUILDERS)
def test_params_overrides(name, int_field, has_reserved):
    build = getattr(lib, name)
    with pytest.raises(TypeError) as e:
        build(no_such_field=1)
    assert str(e.value) == "%s: unknown field 'no_such_field'" % name
    p = build()
    assert hasattr(p, 'reserved') == has_reserved
    with pytest.raises(TypeError) as e:
        build(reserved=0)
    assert str(e.value) == "%s: unknown field 'reserved'" % name
    # a float for an integer field is truncated by int(), an int for a float field becomes a float
    p = build(**{int_field: 3.9})
    assert getattr(p, int_field) == 3 and type(getattr(p, int_field)) is int
    assert getattr(build(**{int_field: -2.5}), int_field) == -2


def test_params_overrides_float_and_unsigned_fields():
    p = lib.plan_params(gamma=1, goal_reward=7)
    assert (p.gamma, p.goal_reward) == (1.0, 7.0) and type(p.gamma) is float
    assert lib.cem_params(seed=2.9).seed == 2
    assert lib.push_proposal_params('episode', step=1.0).step == 1
    with pytest.raises(ValueError):
        lib.plan_params(n_bodies='three')      # (the field's type does the conversion, and refuses as it does)
