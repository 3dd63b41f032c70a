"""Policies (``robovat/policies/*``): ``policy.action(observation) -> action``."""
import numpy as np

from robovat_amd import configs
from robovat_amd.envs.push.heuristic_push_sampler import HeuristicPushSampler


class Policy(object):
    def __init__(self, env, config=None):
        self.env = env
        self.config = config

    def action(self, observation):
        return self._action(observation)


class RandomPolicy(Policy):
    """``env.action_space.sample()`` (random_policy.py:14-23).  With a
    ``VecPushEnv`` the draw happens on the device (rv_policy_random)."""

    def _action(self, observation):
        if hasattr(self.env, 'sample_random_actions'):
            return self.env.sample_random_actions()
        return self.env.action_space.sample()


class HeuristicPushPolicy(Policy):
    """push_policy.py:12-52; batched envs use rv_policy_heuristic."""

    def __init__(self, env, config=None):
        config = config or configs.AttrDict(configs.HEURISTIC_PUSH_POLICY_CONFIG)
        super(HeuristicPushPolicy, self).__init__(env, config)
        self._sampler = HeuristicPushSampler(
            cspace_low=config.ACTION.CSPACE.LOW, cspace_high=config.ACTION.CSPACE.HIGH,
            translation_x=config.ACTION.MOTION.TRANSLATION_X, translation_y=config.ACTION.MOTION.TRANSLATION_Y,
            max_attemps=config.HEURISTICS.MAX_ATTEMPS)

    def _action(self, observation):
        if hasattr(self.env, 'sample_heuristic_actions'):
            return self.env.sample_heuristic_actions(self.config.HEURISTICS.MAX_ATTEMPS)
        return self._sampler.sample(np.asarray(observation['position']), np.asarray(observation['body_mask']),
                                    int(observation['num_episodes']), int(observation['num_steps']), num_samples=1)[0]


class AntipodalGrasp4DofPolicy(Policy):
    """grasp_policy.py:17-75: AntipodalDepthImageGraspSampler on the env's depth image.  Grasp envs sample on the
    device (rv_policy_antipodal); the action is in the env's ACTION.TYPE."""

    def __init__(self, env, config=None):
        config = config or configs.AttrDict(configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG)
        super(AntipodalGrasp4DofPolicy, self).__init__(env, config)

    def _action(self, observation):
        if hasattr(self.env, 'sample_antipodal_actions'):
            depth = None if observation is None else observation.get('depth')
            return self.env.sample_antipodal_actions(depth, self.config)
        raise NotImplementedError('AntipodalGrasp4DofPolicy needs a Grasp4DofEnv / VecGrasp4DofEnv')


class _GraspCandidatePolicy(Policy):
    """What the policies that choose among ``sample_antipodal_candidates`` share.  ``env``: a ``VecGrasp4DofEnv`` or a
    ``Grasp4DofEnv``, refused unless it has the method ``needs``."""

    def __init__(self, env, config, needs):
        config = config or configs.AttrDict(configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG)
        super(_GraspCandidatePolicy, self).__init__(env, config)
        self._vec = getattr(env, '_vec', env)      # (a Grasp4DofEnv is a VecGrasp4DofEnv of one)
        self._single = self._vec is not env
        if not hasattr(self._vec, needs):
            raise NotImplementedError('%s needs a Grasp4DofEnv / VecGrasp4DofEnv' % type(self).__name__)

    def _depth_of(self, observation, render):
        """the observation's depth as [N, H, W]; without one, a render of the world if ``render``, else None"""
        depth = None if observation is None else observation.get('depth')
        if depth is not None and self._single:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        if depth is None and render:
            depth, _ = self._vec.world.render()
        return depth

    def _sample(self, depth):
        """``num_samples`` candidates per env; a single env without one is refused as the reference's sampler refuses"""
        v = self._vec
        cand = v.sample_antipodal_candidates(self.num_samples, depth, self.config)
        if self._single and int(v.antipodal_status[0].item()) != 1:
            raise ValueError('Failed to sample any valid grasp (antipodal status %d).' % int(v.antipodal_status[0].item()))
        return cand

    def _first_index(self, qualifies):
        """[N] the lowest index k at which ``qualifies`` (bool [N, K]) holds, else 0"""
        t = self._vec.world.torch
        n, k = qualifies.shape
        index = t.arange(k, device=qualifies.device)[None, :].expand(n, k)
        first = t.where(qualifies, index, t.full_like(index, k)).min(dim=1).values
        return t.where(first < k, first, t.zeros_like(first))


class LookaheadGrasp4DofPolicy(_GraspCandidatePolicy):
    """AntipodalGrasp4DofPolicy with one step of look-ahead, the simulator as the model: ``num_samples`` distinct
    antipodal grasps per env (``sample_antipodal_candidates``, the reference sampler's ``sample(depth, camera, K)``) are
    each tried on a bit-exact copy of the env (``try_grasps``), and the action is the lowest-index candidate whose
    GraspReward is positive, else candidate 0 -- the grasp AntipodalGrasp4DofPolicy takes.  An env step is deterministic
    given its action, so the env succeeds whenever one of its candidates does.  The action is in the env's ACTION.TYPE
    (an 'IMAGE' env converts it with its nominal camera when it steps; the trial used the env's own calibration).
    Kept: ``last_choice`` [N] and ``last_rewards`` [N, K].  ``env``: a ``VecGrasp4DofEnv`` or a ``Grasp4DofEnv``."""

    def __init__(self, env, num_samples, config=None):
        super(LookaheadGrasp4DofPolicy, self).__init__(env, config, 'try_grasps')
        self.num_samples = int(num_samples)
        if self.num_samples < 1:
            raise ValueError('LookaheadGrasp4DofPolicy: num_samples must be positive')
        self.last_choice = self.last_rewards = None

    def _action(self, observation):
        v = self._vec
        t = v.world.torch
        cand = self._sample(self._depth_of(observation, render=False))      # (no depth: the sampler renders)
        rewards, _ = v.try_grasps(v.antipodal_actions4)
        choice = self._first_index(rewards > 0)      # (the lowest index that succeeds)
        self.last_choice, self.last_rewards = choice, rewards
        actions = cand[t.arange(v.num_envs, device=v.device), choice]
        if self._single:
            self.last_choice, self.last_rewards = int(choice[0]), rewards[0].cpu().numpy()
            return actions[0].cpu().numpy()
        return actions


class GraspQualityPolicy(_GraspCandidatePolicy):
    """AntipodalGrasp4DofPolicy with a learned ranking in place of "the first one": ``num_samples`` distinct antipodal
    grasps per env (``sample_antipodal_candidates``) from one depth image, their grasp-centred crops and the logits of
    ``model`` (``grasp_qualities``: rv_grasp_crops, rv_grasp_quality), and the action is the candidate with the highest
    logit among the rows the sampler found (``antipodal_status == 1`` and k < ``antipodal_count``), the lowest index among
    equals; candidate 0 -- the grasp AntipodalGrasp4DofPolicy takes -- where an env has no such row or its best logit is
    NaN.  Nothing is executed: no ``try_grasps``, no ground-truth state, one render.  The action is in the env's
    ACTION.TYPE.  Kept: ``last_choice`` [N] and ``last_logits`` [N, K].  ``model``: a
    ``perception.grasp_quality.GraspQualityModel``; ``crop``: ``step`` of the crops (default 3).  ``env``: a
    ``VecGrasp4DofEnv`` or a ``Grasp4DofEnv``."""

    def __init__(self, env, model, num_samples, config=None, **crop):
        super(GraspQualityPolicy, self).__init__(env, config, 'grasp_qualities')
        self.model, self.crop = model, dict(crop)
        self.num_samples = int(num_samples)
        if self.num_samples < 1:
            raise ValueError('GraspQualityPolicy: num_samples must be positive')
        self.last_choice = self.last_logits = None

    def _action(self, observation):
        v = self._vec
        t = v.world.torch
        depth = self._depth_of(observation, render=True)      # (one render serves the sampler and the crops)
        cand = self._sample(depth)
        logits = v.grasp_qualities(self.model, v.antipodal_image_grasps, depth, **self.crop)
        index = t.arange(self.num_samples, device=v.device)[None, :]
        valid = (v.antipodal_status == 1)[:, None] & (index < v.antipodal_count[:, None])
        masked = t.where(valid, logits, t.full_like(logits, float('-inf')))
        best = masked.max(dim=1, keepdim=True).values      # (NaN if a valid logit is NaN; -inf without a valid row)
        choice = self._first_index(valid & (masked == best))      # (NaN equals nothing: candidate 0)
        self.last_choice, self.last_logits = choice, logits
        actions = cand[t.arange(v.num_envs, device=v.device), choice]
        if self._single:
            self.last_choice, self.last_logits = int(choice[0]), logits[0].cpu().numpy()
            return actions[0].cpu().numpy()
        return actions


class CEMGraspPolicy(_GraspCandidatePolicy):
    """``GraspQualityPolicy`` with a search around the good candidates: one render, ``num_samples`` (K)
    antipodal candidates (``sample_antipodal_candidates``), then ``num_iterations`` times { score; ``refine_grasps``: keep
    the ``num_elites`` best, resample the rest around them } with the sigmas times ``decay ** t`` in round t, and a final
    scoring.  A last ``refine_grasps`` call with ``num_elites = K`` and zero sigmas sorts the rows, and the action is row 0
    -- the ranking is rv_grasp_refine's (descending, the lower index among equals, NaNs last), no ranking code sits here.
    ``score='model'``: the logits of ``model`` (``grasp_qualities``), nothing is executed; ``score='simulator'``: the
    rewards of ``try_grasps(antipodal_actions4)``, every candidate executed on a copy of its env, no model needed -- how
    far refinement goes with a perfect ranking.  Elites are kept bit for bit, so an env's best score never goes down from
    one scoring to the next.  Where an env has no candidate, or its best score is NaN (every candidate's is), the action
    is candidate 0 of the first sampling, the grasp AntipodalGrasp4DofPolicy takes.  ``num_iterations = 0`` with
    ``score='model'`` is ``GraspQualityPolicy``'s action (which, unlike this one, also falls back to candidate 0 when only
    SOME logit is NaN).  The action is in the env's ACTION.TYPE.  ``num_elites`` None: max(1, K // 4).  The default sigmas
    (3 px, 0.15 rad, 5 mm) and ``decay`` are BUILD-CHOSEN: nobody has measured them.  Kept: ``last_scores``, a list with
    one [N, K] tensor per scoring; ``last_grasps`` [N, K, 5], the sorted final rows; ``last_choice_parentage``, the
    ``refine_parent`` [N, K] of every ``refine_grasps`` call in order (the sort's last), through which row 0 traces back
    to a candidate of the first sampling.  ``crop``: ``step`` of the crops.  ``env``: a ``VecGrasp4DofEnv`` or a
    ``Grasp4DofEnv``."""

    def __init__(self, env, num_samples, num_iterations=2, num_elites=None, model=None, score='model', sigma_center=3.0,
                 sigma_angle=0.15, sigma_depth=0.005, decay=0.5, seed=0, config=None, **crop):
        super(CEMGraspPolicy, self).__init__(env, config, 'refine_grasps')
        self.num_samples, self.num_iterations = int(num_samples), int(num_iterations)
        if self.num_samples < 1 or self.num_iterations < 0:
            raise ValueError('CEMGraspPolicy: num_samples must be positive and num_iterations not negative')
        self.num_elites = max(1, self.num_samples // 4) if num_elites is None else int(num_elites)
        if not 1 <= self.num_elites <= self.num_samples:
            raise ValueError('CEMGraspPolicy: num_elites must be in [1, num_samples]')
        if score not in ('model', 'simulator'):
            raise ValueError("CEMGraspPolicy: score must be 'model' or 'simulator'")
        if score == 'model' and model is None:
            raise ValueError("CEMGraspPolicy: score='model' needs a model")
        self.model, self.score, self.crop = model, score, dict(crop)
        self.sigmas = (float(sigma_center), float(sigma_angle), float(sigma_depth))
        self.decay, self.seed = float(decay), int(seed)
        self.last_scores = self.last_grasps = self.last_choice_parentage = None

    def _scores(self, depth):
        v = self._vec
        if self.score == 'model':
            return v.grasp_qualities(self.model, v.antipodal_image_grasps, depth, **self.crop)
        return v.try_grasps(v.antipodal_actions4)[0]

    def _action(self, observation):
        v = self._vec
        t = v.world.torch
        depth = self._depth_of(observation, render=True)      # (one render serves the sampler, the crops and the refinement)
        first0 = self._sample(depth)[:, 0].clone()
        scores, parents = [], []
        for it in range(self.num_iterations):
            scores.append(self._scores(depth))
            v.refine_grasps(scores[-1], self.num_elites, [s * self.decay ** it for s in self.sigmas], it, depth=depth,
                            config=self.config, seed=self.seed)
            parents.append(v.refine_parent)
        scores.append(self._scores(depth))
        cand = v.refine_grasps(scores[-1], self.num_samples, (0.0, 0.0, 0.0), self.num_iterations, depth=depth,
                               config=self.config, seed=self.seed)
        parents.append(v.refine_parent)
        best = scores[-1].gather(1, v.refine_parent[:, :1].long().clamp(min=0))[:, 0]
        fallback = (v.antipodal_count == 0) | t.isnan(best)
        actions = t.where(fallback[:, None], first0, cand[:, 0])
        self.last_scores, self.last_grasps, self.last_choice_parentage = scores, v.antipodal_image_grasps, parents
        if self._single:
            return actions[0].cpu().numpy()
        return actions


class _LookaheadPushPolicy(Policy):
    """What the look-ahead push policies share: the set-up, the ranking of simulated plans (``_rank``) and the first
    action of the best one (``_first_actions``).  ``env``: a ``VecPushEnv`` or a ``PushEnv``."""

    def __init__(self, env, config, num_samples, horizon, gamma, use_plan_reward, is_high_level):
        super(_LookaheadPushPolicy, self).__init__(env, config)
        if int(num_samples) < 1 or int(horizon) < 1:
            raise ValueError('%s: num_samples and horizon must be positive' % type(self).__name__)
        self._vec = getattr(env, '_vec', env)      # (a PushEnv is a VecPushEnv of one)
        self._single = self._vec is not env
        self.num_samples, self.horizon, self.gamma = int(num_samples), int(horizon), float(gamma)
        self.use_plan_reward, self.is_high_level = bool(use_plan_reward), bool(is_high_level)
        self._torch = self._vec.world.torch

    def _rank(self, states, rewards):
        """(returns [N, S], best int32 [N]): the planning-mode PushReward of ``states`` (``score_plans``, discount
        ``gamma``) with ``use_plan_reward``, else the discounted sum of ``rewards`` [N, S, H]; the lowest index among
        equals"""
        t, v = self._torch, self._vec
        if self.use_plan_reward:
            returns, _, best = v.score_plans(states, None, self.is_high_level, self.gamma)
        else:
            disc = t.full((self.horizon,), self.gamma, device=v.device, dtype=t.float32) ** t.arange(self.horizon, device=v.device)
            returns = (rewards * disc).sum(dim=2)
            best = returns.argmax(dim=1).to(t.int32)      # (the first of equal maxima)
        return returns, best

    def _first_actions(self, cand, best):
        """(step 0 of candidate ``best`` per env, ``best``) -- for a PushEnv one action and an int"""
        t, v = self._torch, self._vec
        actions = cand[t.arange(v.num_envs, device=v.device), best.long(), 0]
        if self._single:
            return actions[0].cpu().numpy(), int(best[0])
        return actions, best

    def _action(self, observation):
        return self.plan(observation)[0]

    def plan(self, observation=None):
        """(actions [N] + action shape, best int32 [N]) -- for a PushEnv one action and an int.  Also kept:
        ``last_best`` and ``last_returns`` [N, S] (and ``last_found`` where the candidates are proposals).  One round of
        candidates from the policy's ``_candidates()`` -> (cand [N, S, H] + action shape, states, rewards, found or
        None), ranked once."""
        cand, states, rewards, found = self._candidates()
        returns, best = self._rank(states, rewards)
        self.last_best, self.last_returns = best, returns
        if found is not None:
            self.last_found = found
        return self._first_actions(cand, best)


class ShootingPushPolicy(_LookaheadPushPolicy):
    """Random-shooting model-predictive control with the simulator as the model: per env ``num_samples`` candidate
    action sequences of ``horizon`` steps, drawn U(-1, 1) from a torch generator seeded with ``seed``, are tried on
    copies of the env in one call (``VecPushEnv.simulate_plans``) and ranked -- by the planning-mode PushReward of the
    simulated states (``score_plans``, discount ``gamma``; ``use_plan_reward=True``) or by the discounted sum of the
    rewards the env itself gave along the way.  The action is the first one of the best sequence, the lowest index
    among equals; the env does not change.  ``env``: a ``VecPushEnv`` or a ``PushEnv``."""

    def __init__(self, env, num_samples, horizon, gamma=1.0, seed=0, use_plan_reward=True, is_high_level=False, config=None):
        super(ShootingPushPolicy, self).__init__(env, config, num_samples, horizon, gamma, use_plan_reward, is_high_level)
        self._gen = self._torch.Generator(device=self._vec.device)
        self.reseed(seed)
        self.last_best = self.last_returns = None

    def reseed(self, seed):
        """start the candidate stream over: the same seed gives the same candidates again"""
        self._gen.manual_seed(int(seed))

    def _candidates(self):
        t, v = self._torch, self._vec
        shape = (v.num_envs, self.num_samples, self.horizon) + tuple(v.action_shape)
        cand = t.rand(shape, generator=self._gen, device=v.device, dtype=t.float32) * 2.0 - 1.0
        states, rewards, _ = v.simulate_plans(cand)
        return cand, states, rewards, None


class HeuristicShootingPushPolicy(_LookaheadPushPolicy):
    """``ShootingPushPolicy`` with informed candidates: per env ``num_samples`` plans of ``horizon`` aimed pushes
    (``VecPushEnv.propose_plans``: every push starts ``start_margin`` clear of the bodies and touches one of them within
    ``motion_margin``, candidate k aiming at body k % n_bodies, each step drawn from the simulated state its plan has
    reached; Philox keyed by the world's seed, the global env id, the env.step() being planned, the step of the plan,
    ``seed`` and k -- an env plans the same whatever else is in the batch, and the same again until it steps) are tried
    on copies of the env and ranked exactly as ``ShootingPushPolicy`` ranks them: ``score_plans`` with discount
    ``gamma``, or the discounted rewards the env gave.  The action is the first one of the best plan, the lowest index
    among equals; the env does not change.  Kept: ``last_best`` [N], ``last_returns`` [N, S] and ``last_found``
    [N, S, H] (False where a push ran out of ``max_attempts``).  ``env``: a ``VecPushEnv`` or a ``PushEnv``."""

    def __init__(self, env, num_samples, horizon, gamma=1.0, seed=0, max_attempts=20000, start_margin=0.05,
                 motion_margin=0.01, use_plan_reward=True, is_high_level=False, config=None):
        super(HeuristicShootingPushPolicy, self).__init__(env, config, num_samples, horizon, gamma, use_plan_reward, is_high_level)
        self.seed = int(seed)
        self.max_attempts, self.start_margin, self.motion_margin = int(max_attempts), float(start_margin), float(motion_margin)
        self.last_best = self.last_returns = self.last_found = None

    def _candidates(self):
        cand, states, rewards, _, found = self._vec.propose_plans(self.num_samples, self.horizon, self.seed, self.max_attempts,
                                                                  self.start_margin, self.motion_margin)
        return cand, states, rewards, found


class RouteShootingPushPolicy(_LookaheadPushPolicy):
    """``HeuristicShootingPushPolicy`` with candidates that know the layout: per env ``num_samples`` plans of ``horizon``
    pushes that move body 0, the task's target, one cell along the tiles towards the goal
    (``VecPushEnv.propose_route_plans``: candidate 0 is the push without jitter, the others vary its direction, back-off,
    side offset and length; each step is drawn from the simulated state its plan has reached; keyed as the heuristic
    proposals are) are tried on copies of the env and ranked exactly as ``ShootingPushPolicy`` ranks them: ``score_plans``
    with discount ``gamma``, or the discounted rewards the env gave.  The action is the first one of the best plan, the
    lowest index among equals; the env does not change.  ``route``: fields of ``lib.push_route_params`` (max_attempts,
    keep_nominal, start_margin, angle_jitter, back_lo, back_hi, lateral, length_lo, length_hi).  Kept: ``last_best``
    [N], ``last_returns`` [N, S] and ``last_found`` [N, S, H].  Crossing and insertion tasks only.  ``env``: a
    ``VecPushEnv`` or a ``PushEnv``."""

    def __init__(self, env, num_samples, horizon, gamma=1.0, seed=0, use_plan_reward=True, is_high_level=False, config=None,
                 **route):
        super(RouteShootingPushPolicy, self).__init__(env, config, num_samples, horizon, gamma, use_plan_reward, is_high_level)
        self.seed = int(seed)
        self.route = dict(route)
        self.last_best = self.last_returns = self.last_found = None

    def _candidates(self):
        cand, states, rewards, _, found = self._vec.propose_route_plans(self.num_samples, self.horizon, self.seed, **self.route)
        return cand, states, rewards, found


class CEMPushPolicy(_LookaheadPushPolicy):
    """Cross-entropy-method model-predictive control with the simulator as the model.  Per env a normal distribution over
    action sequences of ``horizon`` steps starts at mean 0, std ``init_std``; ``num_iterations`` times, ``num_samples``
    candidates are drawn from it on the device (``VecPushEnv.sample_plan_candidates``: Philox keyed by the world's seed,
    the global env id, the env.step() being planned, the iteration and ``seed`` -- an env plans the same whatever else is
    in the batch), tried on copies of the env (``simulate_plans``), ranked as ``ShootingPushPolicy`` ranks them
    (``score_plans`` with discount ``gamma``, or the discounted rewards the env gave), and the distribution is refit to
    the ``num_elites`` best (default max(1, S // 8); ``refit_plan_distribution`` with smoothing ``alpha`` and the floor
    ``min_std``).  With ``keep_mean`` candidate 0 of every iteration is the current mean.  The action is the first step
    of the best-returning candidate seen in ANY iteration: the lowest iteration, then the lowest index among equals.
    With ``warm_start`` the next call starts from this call's final mean shifted by one step (zeros in the last step, std
    back to ``init_std``); ``reset(mask)`` forgets it for envs whose episode restarted.  The env does not change.
    ``env``: a ``VecPushEnv`` or a ``PushEnv``."""

    def __init__(self, env, num_samples, horizon, num_iterations=3, num_elites=None, gamma=1.0, init_std=0.5, min_std=0.05,
                 alpha=0.0, seed=0, keep_mean=True, warm_start=True, use_plan_reward=True, is_high_level=False, config=None):
        if int(num_samples) < 1 or int(horizon) < 1 or int(num_iterations) < 1:
            raise ValueError('CEMPushPolicy: num_samples, horizon and num_iterations must be positive')
        super(CEMPushPolicy, self).__init__(env, config, num_samples, horizon, gamma, use_plan_reward, is_high_level)
        self.num_iterations = int(num_iterations)
        self.num_elites = max(1, self.num_samples // 8) if num_elites is None else int(num_elites)
        if not 1 <= self.num_elites <= self.num_samples:
            raise ValueError('CEMPushPolicy: num_elites must be in [1, num_samples]')
        self.init_std, self.min_std, self.alpha = float(init_std), float(min_std), float(alpha)
        self.seed, self.keep_mean, self.warm_start = int(seed), bool(keep_mean), bool(warm_start)
        self._warm = None      # the next call's initial mean, [N, H] + action shape
        self.last_mean = self.last_std = self.last_returns = self.last_best = None

    def reset(self, mask=None):
        """forget the warm start: of every env, or of those flagged in ``mask`` (bool [N]) -- their next plan starts at 0"""
        if mask is None or self._warm is None:
            self._warm = None
            return
        t = self._torch
        m = t.as_tensor(mask, device=self._vec.device).reshape(self._vec.num_envs).bool()
        self._warm = t.where(m.reshape((-1,) + (1,) * (self._warm.dim() - 1)), t.zeros_like(self._warm), self._warm)

    def initial_mean(self):
        """the mean the next ``plan()`` starts from, [N, H] + action shape"""
        t, v = self._torch, self._vec
        if self.warm_start and self._warm is not None:
            return self._warm.clone()
        return t.zeros((v.num_envs, self.horizon) + tuple(v.action_shape), dtype=t.float32, device=v.device)

    def plan(self, observation=None):
        """(actions [N] + action shape, (iteration int32 [N], index int32 [N]) of the chosen candidates) -- for a PushEnv
        one action and two ints.  Also kept: ``last_mean`` / ``last_std`` [N, H] + action shape (the final distribution),
        ``last_returns`` [I, N, S] and ``last_best`` (what is returned second)."""
        t, v = self._torch, self._vec
        n = v.num_envs
        mean = self.initial_mean()
        std = t.full_like(mean, self.init_std)
        rows = t.arange(n, device=v.device)
        all_returns = []
        best_val = best_it = best_idx = best_act = None
        for it in range(self.num_iterations):
            cand = v.sample_plan_candidates(mean, std, self.num_samples, it, self.seed, self.keep_mean)
            states, rewards, _ = v.simulate_plans(cand)
            returns, best = self._rank(states, rewards)
            val, act = returns[rows, best.long()], cand[rows, best.long(), 0]
            if it == 0:
                best_val, best_idx, best_act = val, best, act
                best_it = t.zeros_like(best)
            else:
                better = val > best_val      # (strictly: the lowest iteration among equals)
                best_val = t.where(better, val, best_val)
                best_idx = t.where(better, best, best_idx)
                best_it = t.where(better, t.full_like(best_it, it), best_it)
                best_act = t.where(better.reshape((-1,) + (1,) * (act.dim() - 1)), act, best_act)
            all_returns.append(returns)
            mean, std, _ = v.refit_plan_distribution(cand, returns, mean, std, self.num_elites, self.alpha, self.min_std)
        self.last_mean, self.last_std, self.last_returns = mean, std, t.stack(all_returns, dim=0)
        self.last_best = (best_it, best_idx)
        if self.warm_start:
            self._warm = t.cat([mean[:, 1:], t.zeros_like(mean[:, :1])], dim=1)
        if self._single:
            self.last_best = (int(best_it[0]), int(best_idx[0]))
            return best_act[0].cpu().numpy(), self.last_best
        return best_act, self.last_best
