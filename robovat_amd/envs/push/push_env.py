"""PushEnv on the MI355X backend.

``VecPushEnv`` is the fast path: N envs advance together, ``step(actions)`` is
one ``rv_step_macro`` launch that runs the whole ``_execute_action`` phase
machine, the settle, the observations and the reward on the device
(reference: ``robovat/envs/push/push_env.py:599-937``,
``robovat/envs/robot_env.py:204-312``).  ``PushEnv`` keeps the reference's
single-env gym-style API (``reset() -> obs``, ``step(a) -> obs, reward, done,
None``, same observation keys / dtypes / shapes, ``push_env.py:169-267``) as a
batch of one.
"""
import collections

import numpy as np

from robovat_amd import abi, configs, scenes


class Box(object):
    """Stand-in for ``gym.spaces.Box`` (gym is not a dependency)."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.low = np.broadcast_to(np.asarray(low, dtype=dtype), shape if shape is not None else np.shape(low)).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=dtype), self.low.shape).copy()
        self.shape, self.dtype = self.low.shape, dtype

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


class VecPushEnv(object):
    """N PushEnv instances on one GPU (env shards [offset, offset + N))."""

    def __init__(self, num_envs, config=None, robot_config=None, device=0, seed=0,
                 env_id_offset=0, use_point_cloud=False, physics=None):
        from robovat_amd import lib
        self.config = config or configs.push_env_config()
        self.robot_config = robot_config or configs.sawyer_config()
        self._owns_world = physics is None
        self._physics = physics
        if physics is None:
            self.scene, self.shape_names = scenes.make_scene()
            self.rv_config = configs.make_rv_config(self.config, self.robot_config, self.shape_names,
                                                    n_envs=num_envs, env_id_offset=env_id_offset, seed=seed)
            self.world = lib.World(self.rv_config, self.scene, device=device)
        else:
            # the env runs on the world of a Simulator's physics backend (HipPhysics): what the env
            # does is visible through the Simulator / Body API and the other way round
            assert int(num_envs) == 1, 'a Simulator holds one env'
            self._physics = physics
            physics.configure(self.config, self.robot_config, seed=seed, worker_id=env_id_offset)
            self.scene, self.shape_names = physics.scene, physics.shape_names
            self.world, self.rv_config = physics.world, physics.rv_config
        self.num_envs = int(num_envs)
        self.max_movable_bodies = abi.RV_MAXB
        self.use_point_cloud = bool(use_point_cloud)
        g = self.rv_config.num_goal_steps
        self.action_shape = (4,) if g == 0 else (g, 4)
        self.action_space = Box(-1.0, 1.0, self.action_shape)
        self._macro_index = 0
        self._plan_worlds = {}      # S -> the world of N x S envs that simulate_plans branches into
        from robovat_amd.envs import recording
        self._recorder = recording.make_recorder(self)      # config.RECORDING (None: off, the default)

    @property
    def device(self):
        return self.world.device

    def get_observation(self):
        return self.world.observe(point_cloud=self.use_point_cloud)

    def camera_calibration(self):
        """(intrinsics [N, 3, 3], translation [N, 3], rotation [N, 3, 3]) of the simulated Kinect2 of every env: the
        configured calibration plus the uniform noise ArmEnv._reset_camera draws at each reset (arm_env.py:109-152;
        KINECT2.DEPTH.INTRINSICS_NOISE / TRANSLATION_NOISE / ROTATION_NOISE, push_env.py:273-280)."""
        cam = self.world.camera().cpu().numpy()
        k = np.zeros((self.num_envs, 3, 3), np.float32)
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 0, 1], k[:, 2, 2] = cam[:, 0], cam[:, 1], cam[:, 2], cam[:, 3], cam[:, 4], 1.0
        return k, cam[:, 14:17].copy(), cam[:, 5:14].reshape(-1, 3, 3).copy()

    def reset(self, mask=None):
        """RobotEnv.reset for every env (or the masked ones)."""
        self.world.reset(mask)
        if self._physics is not None:
            self._physics.on_env_reset()
        if self._recorder is not None:
            self._recorder.on_reset(mask)
        return self.get_observation()

    def step(self, actions):
        """RobotEnv.step for every env whose episode is not done.  With ``config.RECORDING.USE`` the step goes through
        ``record_step`` and the frames of the recorded envs go to their episode files (``envs/recording.py``)."""
        if self._recorder is not None:
            return self._recorder.step(actions)
        return self._plain_step(actions)

    def _world_actions(self, actions):
        """the actions as the world takes them: float32 [N, G, 4] on the device"""
        return self.world._in(actions, (self.num_envs, self.world.G, 4), self.world.torch.float32)

    def record_step(self, actions, cameras, env_index, every, height=None, width=None, supersample=1, max_frames=256):
        """``step(actions)`` watched through free cameras (``envs.recording.record_step``): returns (obs, reward, done,
        {'frames' uint8 [T, V, H, W, 3], 'sim_steps' int32 [T, V], 'num_frames'}) -- a frame of every view before the first
        substep, then at most ``every`` (>= 2) substeps apart, and of the completed state.  The first three are ``step()``'s bit for bit."""
        from robovat_amd.envs import recording
        return recording.record_step(self, actions, cameras, env_index, every, height, width, supersample, max_frames)

    def _plain_step(self, actions):
        self.world.set_actions(actions)
        self.world.step_macro()
        self._macro_index += 1
        obs = self.get_observation()
        reward, done = self.world.reward()
        return obs, reward, done.bool(), None

    def sample_random_actions(self):
        """RandomPolicy on the device (Philox keyed by global env id and step)."""
        a = self.world.policy_random(self._macro_index)
        return a.reshape((self.num_envs,) + self.action_shape)

    def sample_heuristic_actions(self, max_attempts=20000):
        a = self.world.policy_heuristic(max_attempts)
        return a.reshape((self.num_envs,) + self.action_shape)

    def contact_points(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1, capacity=abi.RV_CP_MAX):
        """PyBullet contact records of every env on the device (``lib.World.contact_points``): ids [N, P, 4],
        data [N, P, RV_CP_NF], count [N]; bodies are slots, ``abi.RV_CP_TABLE`` or ``abi.RV_CP_ARM``."""
        return self.world.contact_points(body_a, link_a, body_b, link_b, capacity)

    def contact_forces(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1):
        """Net contact force on body A, [N, 3] on the device (``lib.World.contact_forces``)."""
        return self.world.contact_forces(body_a, link_a, body_b, link_b)

    def _plan_params(self, n_bodies, is_high_level, gamma=1.0):
        from robovat_amd import lib
        return lib.plan_params(n_bodies=n_bodies, is_high_level=int(bool(is_high_level)), gamma=gamma)

    def score_plans(self, plans, state=None, is_high_level=False, gamma=1.0):
        """Planning-mode PushReward (``get_reward_fn(task, layout, is_planning=True)``) over S candidate plans of H
        steps per env, on the device: ``plans`` [N, S, H, B, 2] (or [..., 3] positions, z dropped) are the states after
        each step, ``state`` [N, B, 2] the state before the first (None: the last observation).  Returns (returns [N, S]
        -- the rewards up to and including the first terminating step, discounted by ``gamma`` --, lengths [N, S], best
        [N]: the plan with the largest return, the first among equals)."""
        b = int(self.world.torch.as_tensor(plans).shape[-2])
        return self.world.plan_score(plans, state, self._plan_params(b, is_high_level, gamma))

    def plan_rewards(self, state, next_state, is_high_level=False):
        """Planning-mode PushReward of M transitions on the device: ``state`` / ``next_state`` [M, B, 2] (or [M, B, 3]).
        Returns (reward float32 [M], termination bool [M])."""
        b = int(self.world.torch.as_tensor(state).shape[-2])
        r, t = self.world.plan_reward(state, next_state, self._plan_params(b, is_high_level))
        return r, t.bool()

    def save_state(self):
        """All N envs as they are now (``lib.World.save_state``): a ``lib.Snapshot`` on the device, plus the index of the
        env's next RandomPolicy draw.  An env.step() that ``step_poll`` left unfinished is part of the state."""
        snap = self.world.save_state()
        snap.macro_index = self._macro_index
        return snap

    def restore_state(self, snap, mask=None):
        """Put the envs back where ``snap`` was taken: all of them, or those flagged in ``mask`` (bool [N]; the others
        keep their present state).  From then on they continue bit for bit as they did after the snapshot.  (For an env
        that lives in a Simulator, the host-side Body / Constraint wrappers are not part of a snapshot.)"""
        if mask is None:
            self.world.load_state(snap)
            if getattr(snap, 'macro_index', None) is not None:
                self._macro_index = snap.macro_index
            return
        torch = self.world.torch
        m = torch.as_tensor(mask, device=self.device).reshape(self.num_envs).bool()
        ar = torch.arange(self.num_envs, device=self.device, dtype=torch.int32)
        self.world.load_state(snap, torch.where(m, ar, torch.full_like(ar, -1)))

    def _plan_world(self, s):
        """the world of N x S envs behind simulate_plans: made on first use and kept per S; same scene, config and seed
        (rv_create picks the env-kernel build for its size)"""
        w = self._plan_worlds.get(int(s))
        if w is None:
            from robovat_amd import lib
            cfg = abi.rv_config.from_buffer_copy(bytes(self.rv_config))
            cfg.n_envs = self.num_envs * int(s)
            cfg.env_id_offset = int(self.rv_config.env_id_offset) * int(s)
            w = self._plan_worlds[int(s)] = lib.World(cfg, self.scene, device=self.world.device_index)
        return w

    def simulate_plans(self, actions):
        """Look ahead with the simulator: ``actions`` [N, S, H, G, 4] ([N, S, H, 4] without goal steps) are S candidate
        action sequences of H steps for every env.  Each is tried on a copy of the env (``lib.World.plan_simulate``);
        the envs themselves do not change.  Returns (states float32 [N, S, H, RV_MAXB, 2]: the observed xy of the bodies
        after every step, the ``plans`` of ``score_plans``; rewards float32 [N, S, H]; dones bool [N, S, H]).  A
        candidate whose episode ends early repeats its last state with reward 0, done."""
        a = self.world.torch.as_tensor(actions)
        if a.dim() < 2 or int(a.shape[1]) < 1:
            raise ValueError('simulate_plans: actions must be [N, S, H, G, 4]')
        st, r, d = self._plan_world(int(a.shape[1])).plan_simulate(self.world, a)
        return st, r, d.bool()

    def sample_plan_candidates(self, mean, std, num_samples, iteration, seed=0, keep_mean=True):
        """``num_samples`` candidate plans per env from the normal distribution ``mean`` / ``std`` ([N, H] + action
        shape), clamped to the action space (``lib.World.cem_sample``).  A draw is keyed by the world's seed, the global
        env id, the index of the env.step() being planned, ``iteration``, ``seed``, the candidate and the float: the
        same whatever else is in the batch.  With ``keep_mean`` candidate 0 is the clamped mean.  Returns float32
        [N, S, H] + action shape, the ``actions`` of ``simulate_plans``."""
        from robovat_amd import lib
        m = self.world.torch.as_tensor(mean)
        if m.dim() != 2 + len(self.action_shape) or tuple(m.shape[2:]) != tuple(self.action_shape):
            raise ValueError('sample_plan_candidates: mean and std must be [N, H] + %s' % (tuple(self.action_shape),))
        h = int(m.shape[1])
        p = lib.cem_params(plan_index=self._macro_index, iteration=int(iteration), seed=int(seed) & 0xFFFFFFFF, keep_mean=int(bool(keep_mean)))
        a = self.world.cem_sample(m, std, p, int(num_samples), h)
        return a.reshape((self.num_envs, int(a.shape[1]), h) + self.action_shape)

    def refit_plan_distribution(self, candidates, returns, mean, std, num_elites, alpha=0.0, min_std=0.0):
        """Fit ``mean`` / ``std`` ([N, H] + action shape) to the ``num_elites`` candidates ([N, S, H] + action shape) with
        the largest ``returns`` [N, S] (``lib.World.cem_refit``): ranked descending, the lower index first among equals,
        NaNs last; new = alpha * old + (1 - alpha) * (the elites' mean / standard deviation), the std not below
        ``min_std``.  Returns (mean, std, elite int32 [N, E] by rank); the arguments stay as they are."""
        from robovat_amd import lib
        t = self.world.torch
        c = t.as_tensor(candidates, dtype=t.float32, device=self.device)
        if c.dim() != 3 + len(self.action_shape) or tuple(c.shape[3:]) != tuple(self.action_shape):
            raise ValueError('refit_plan_distribution: candidates must be [N, S, H] + %s' % (tuple(self.action_shape),))
        c = c.reshape(tuple(c.shape[:3]) + (self.world.G, 4))
        p = lib.cem_params(plan_index=self._macro_index, n_elites=int(num_elites), alpha=float(alpha), min_std=float(min_std))
        return self.world.cem_refit(c, returns, mean, std, p)

    def _proposal_params(self, mode, step, seed, max_attempts, start_margin, motion_margin):
        """the key of an env's proposals: 'spread' draws are keyed by the index of the env.step() being planned, 'episode'
        draws by the observation's counters alone (the library refuses a step or seed there)"""
        from robovat_amd import lib
        spread = mode in ('spread', abi.RV_HP_SPREAD)
        return lib.push_proposal_params(mode, plan_index=self._macro_index if spread else 0, step=int(step),
                                        seed=int(seed) & 0xFFFFFFFF, max_attempts=int(max_attempts),
                                        start_margin=float(start_margin), motion_margin=float(motion_margin))

    def _candidates_out(self, out):
        """(actions [M, s, G, 4], status) of ``lib.World.policy_*_multi`` -> (actions [N, S] + action shape, found bool)"""
        a, st = out
        return a.reshape((self.num_envs, int(a.shape[1])) + self.action_shape), st == abi.RV_HP_FOUND

    def _plans_out(self, out):
        """the five tensors of ``lib.World.plan_propose*`` -> (actions [N, S, H] + action shape, states, rewards, dones
        bool, found bool)"""
        a, st, r, d, status = out
        return a.reshape(tuple(a.shape[:3]) + self.action_shape), st, r, d.bool(), status == abi.RV_HP_FOUND

    def sample_heuristic_candidates(self, num_samples, mode='spread', step=0, seed=0, max_attempts=20000,
                                    start_margin=0.05, motion_margin=0.01):
        """``num_samples`` aimed pushes per env from the last observation (``lib.World.policy_heuristic_multi``): each starts
        ``start_margin`` clear of every body and touches its target body within ``motion_margin``.  ``mode`` 'spread':
        candidate k aims at body k % n_bodies in any direction, keyed by the world's seed, the global env id, the index
        of the env.step() being planned, ``step``, ``seed`` and k -- the same whatever else is in the batch.  'episode':
        the reference's ``HeuristicPushSampler.sample(..., num_samples)``, candidate 0 being ``sample_heuristic_actions``'
        push.  Returns (actions float32 [N, S] + action shape, found bool [N, S]: False where ``max_attempts`` ran out
        and the last attempt is returned as drawn)."""
        p = self._proposal_params(mode, step, seed, max_attempts, start_margin, motion_margin)
        return self._candidates_out(self.world.policy_heuristic_multi(p, int(num_samples)))

    def propose_plans(self, num_samples, horizon, seed=0, max_attempts=20000, start_margin=0.05, motion_margin=0.01):
        """Look ahead with aimed pushes: ``num_samples`` plans of ``horizon`` steps per env, tried on copies of the env
        (``lib.World.plan_propose``).  Step t of a plan is the 'spread' candidate of ``sample_heuristic_candidates`` drawn
        from that copy's own state after step t - 1, so every push of a plan aims at where the bodies then are.  The
        envs themselves do not change.  Returns (actions float32 [N, S, H] + action shape, states, rewards, dones as
        ``simulate_plans``, found bool [N, S, H])."""
        if int(num_samples) < 1:
            raise ValueError('propose_plans: num_samples must be positive')
        p = self._proposal_params('spread', 0, seed, max_attempts, start_margin, motion_margin)
        return self._plans_out(self._plan_world(int(num_samples)).plan_propose(self.world, p, int(num_samples), int(horizon)))

    def _route_params(self, step, seed, route):
        """``route``: fields of ``lib.push_route_params`` (max_attempts, keep_nominal, start_margin, angle_jitter, back_lo,
        back_hi, lateral, length_lo, length_hi); the key is that of the 'spread' proposals"""
        from robovat_amd import lib
        for k in ('plan_index', 'step', 'seed', 'copies'):
            if k in route:
                raise TypeError('route proposals: %r is set by the env' % (k,))
        return lib.push_route_params(plan_index=self._macro_index, step=int(step), seed=int(seed) & 0xFFFFFFFF, **route)

    def sample_route_candidates(self, num_samples, step=0, seed=0, **route):
        """``num_samples`` pushes per env that move body 0 -- the target of the crossing and insertion tasks -- one cell
        along the layout towards the goal, from the last observation (``lib.World.policy_route_multi``).  Candidate 0 is
        the push without jitter (``keep_nominal``); the others draw a direction, a back-off, a side offset and a length
        around it, keyed as the 'spread' candidates of ``sample_heuristic_candidates``.  ``route``: the fields of
        ``lib.push_route_params``.  Returns (actions float32 [N, S] + action shape, found bool [N, S]: False where no
        attempt started ``start_margin`` clear of every body)."""
        p = self._route_params(step, seed, route)
        return self._candidates_out(self.world.policy_route_multi(p, int(num_samples)))

    def propose_route_plans(self, num_samples, horizon, seed=0, **route):
        """``propose_plans`` with the pushes of ``sample_route_candidates`` (``lib.World.plan_propose_route``): step t of a
        plan aims from where body 0 is in that copy after step t - 1.  The envs themselves do not change.  Returns
        (actions float32 [N, S, H] + action shape, states, rewards, dones as ``simulate_plans``, found bool [N, S, H])."""
        if int(num_samples) < 1:
            raise ValueError('propose_route_plans: num_samples must be positive')
        p = self._route_params(0, seed, route)
        return self._plans_out(self._plan_world(int(num_samples)).plan_propose_route(self.world, p, int(num_samples), int(horizon)))

    def clustered_point_cloud(self, num_points=None, draw_index=0, chunk=256, depth=None, labels=False, grouping='largest',
                              num_neighbors=100, **overrides):
        """The point clouds as the reference's real-sensor branch makes them (SegmentedPointCloudObs without a simulator,
        camera_obs.py:182-211): render -> deproject -> plane removal -> DBSCAN -> the ``num_clusters`` largest clusters
        sampled to ``num_points`` points (``lib.World.clustered_point_cloud``), ``chunk`` envs at a time.
        ``num_points``: None for the config's; ``overrides``: fields of ``lib.segment_params`` (eps, min_samples,
        plane_thresh, num_hypotheses, num_clusters).  Returns a dict of device tensors: clouds float32 [N, C, P, 3] and
        the diagnostics slot_labels, slot_counts [N, C], plane [N, 4], info [N, 8] (``abi.RV_SEG_INFO_*``; flag
        RV_SEG_FLAG_FEWER: fewer clusters than slots, e.g. bodies that touch), labels [N, H * W] when asked for.
        ``grouping='ward'``: the reference's second ``cluster()`` call after DBSCAN -- Ward agglomeration of the clustered
        points on their ``num_neighbors``-nearest-neighbour graph into exactly ``num_clusters`` groups (``rv_ward_groups``,
        DESIGN.md §26): clouds and slot_counts are then those groups', ward_info [N, 8] (``abi.RV_WARD_INFO_*``) is added,
        and groups [N, H * W] with the labels."""
        from robovat_amd import lib
        if grouping not in ('largest', 'ward'):
            raise ValueError('Unrecognized grouping: %r.' % (grouping,))
        p = lib.segment_params(num_points=int(self.rv_config.num_points) if num_points is None else int(num_points),
                               draw_index=int(draw_index), **overrides)
        ward = None
        if grouping == 'ward':
            ward = lib.ward_params(num_points=int(p.num_points), num_groups=int(p.num_clusters), num_neighbors=int(num_neighbors),
                                   draw_index=int(draw_index))
        return self.world.clustered_point_cloud(p, chunk=chunk, depth=depth, labels=labels, ward=ward)

    def rollout(self, n_steps, auto_reset=True, record=True):
        before =self.world.env_counters().cpu().numpy()[:, [2, 4]] if (auto_reset and self._physics is not None) else None
        out = self.world.rollout(n_steps, self._macro_index, auto_reset, record)
        if before is not None:
            # the host mirror of the user constraints is dropped only when an env really was reset
            # -- every episode end is followed by a reset at the env's NEXT step, so resets = (done before) + (episodes
            # ended) - (done after): an episode that merely ends on the last step of the rollout has not been reset yet,
            # its constraints are still active on the device and the mirror must keep them
            after = self.world.env_counters().cpu().numpy()[:, [2, 4]]
            resets = (before[:, 1] != 0).astype(int) + (after[:, 0] - before[:, 0]) - (after[:, 1] != 0).astype(int)
            if (resets > 0).any():
                self._physics.on_env_reset()
        self._macro_index += int(n_steps)
        return out

    def stats(self):
        return self.world.stats()

    def close(self):
        from robovat_amd.envs import recording
        if self._recorder is not None:
            self._recorder.close()
        recording.close_record_worlds(self)
        for w in self._plan_worlds.values():
            w.close()
        self._plan_worlds = {}
        if self._owns_world:
            self.world.close()


class PushEnv(object):
    """Single-env PushEnv with the reference's API (a VecPushEnv of one)."""

    def __init__(self, simulator=None, config=None, debug=False, robot_config=None, device=0, seed=0,
                 worker_id=0):
        self._config = config or configs.push_env_config()
        self._debug = debug
        # PushEnv(simulator, config) as in the reference (push_env.py:43-48): the env lives in the
        # simulator's physics backend -- bodies, constraints and getters of that Simulator see it
        self._simulator = simulator
        physics = None
        if simulator is not None:
            physics = simulator.physics
            if not hasattr(physics, 'configure'):
                raise ValueError('PushEnv needs a Simulator whose physics backend is HipPhysics')
            if simulator.bodies or simulator.constraints:
                # configure() recreates the world: bodies / constraints added before would silently vanish
                raise ValueError('PushEnv(simulator): the Simulator already holds %d bodies / %d constraints; give the env '
                                 'an empty Simulator' % (len(simulator.bodies), len(simulator.constraints)))
        self._vec = VecPushEnv(1, self._config, robot_config, device=device, seed=seed, env_id_offset=worker_id,
                               use_point_cloud=True, physics=physics)
        self.max_movable_bodies = abi.RV_MAXB
        self.task_name = self._config.TASK_NAME
        self.layout_id = self._config.LAYOUT_ID
        self.num_goal_steps = self._config.NUM_GOAL_STEPS
        self.action_space = self._vec.action_space
        self.phase_list = list(abi.PHASES)
        self._obs_data = self._prev_obs_data = None
        self._done = True
        self._episode_reward = self._total_reward = 0.0

    config = property(lambda s: s._config)
    debug = property(lambda s: s._debug)
    simulator = property(lambda s: s._simulator)
    is_simulation = property(lambda s: True)
    obs_data = property(lambda s: s._obs_data)
    prev_obs_data = property(lambda s: s._prev_obs_data)
    done = property(lambda s: s._done)
    episode_reward = property(lambda s: s._episode_reward)
    total_reward = property(lambda s: s._total_reward)
    info = property(lambda s: {'name': 'PushEnv'})

    def _counters(self):
        return self._vec.world.env_counters().cpu().numpy()[0]

    num_steps = property(lambda s: int(s._counters()[1]))
    num_episodes = property(lambda s: int(s._counters()[2]))

    def _convert(self, obs):
        out = collections.OrderedDict()
        for key in ('num_episodes', 'num_steps', 'layout_id'):
            out[key] = np.array(obs[key][0].item(), dtype=np.int64)
        out['body_mask'] = obs['body_mask'][0].cpu().numpy().astype(np.float32)
        out['point_cloud'] = obs['point_cloud'][0].cpu().numpy().astype(np.float32)
        if self._config.USE_PRESTIGE_OBS:
            out['position'] = obs['position'][0].cpu().numpy().astype(np.float32)
            out['is_safe'] = np.array(obs['is_safe'][0].item(), dtype=np.int64)
            out['is_effective'] = np.array(obs['is_effective'][0].item(), dtype=np.int64)
        return out

    def reset(self):
        self._prev_obs_data = None
        if self._simulator is not None:
            # RobotEnv.reset -> simulator.reset() (robot_env.py:204-237): the episode's Body / Constraint wrappers go
            self._simulator._bodies.clear(); self._simulator._constraints.clear()
        self._obs_data = self._convert(self._vec.reset())
        self._done = False
        self._episode_reward = 0.0
        return self._obs_data

    def step(self, action):
        if self._done:
            raise ValueError('The environment is done. Forget to reset?')
        action = np.asarray(action, dtype=np.float32).reshape((1,) + self._vec.action_shape)
        return self._took(self._vec.step(action))

    def _took(self, out):
        """the bookkeeping of one step of the batch of one; the fourth entry is passed through"""
        obs, reward, done, info = out
        self._prev_obs_data, self._obs_data = self._obs_data, self._convert(obs)
        reward = float(reward[0].item())
        self._done = bool(done[0].item())
        self._episode_reward += reward
        if self._done:
            self._total_reward += self._episode_reward
        return self._obs_data, reward, self._done, info

    def record_step(self, action, cameras, every, height=None, width=None, supersample=1, max_frames=256):
        """``step(action)`` watched through ``cameras`` (``VecPushEnv.record_step`` for this env): the fourth entry is
        {'frames' uint8 [T, V, H, W, 3], 'sim_steps' int32 [T, V], 'num_frames'}."""
        if self._done:
            raise ValueError('The environment is done. Forget to reset?')
        action = np.asarray(action, dtype=np.float32).reshape((1,) + self._vec.action_shape)
        return self._took(self._vec.record_step(action, cameras, [0], every, height, width, supersample, max_frames))

    def get_observation(self):
        return self._obs_data

    def score_plans(self, plans, state=None, is_high_level=False, gamma=1.0):
        """``VecPushEnv.score_plans`` for this env: ``plans`` [S, H, B, 2] (or [1, S, H, B, 2]), ``state`` [B, 2]."""
        torch = self._vec.world.torch
        plans = torch.as_tensor(plans)
        if plans.dim() == 4:
            plans = plans[None]
        if state is not None:
            state = torch.as_tensor(state)
            state = state[None] if state.dim() == 2 else state
        ret, ln, best = self._vec.score_plans(plans, state, is_high_level, gamma)
        return ret[0], ln[0], best[0]

    def plan_rewards(self, state, next_state, is_high_level=False):
        return self._vec.plan_rewards(state, next_state, is_high_level)

    def save_state(self):
        """``VecPushEnv.save_state`` plus what this wrapper keeps on the host (observations, done flag, returns)."""
        snap = self._vec.save_state()
        snap.host = (self._obs_data, self._prev_obs_data, self._done, self._episode_reward, self._total_reward)
        return snap

    def restore_state(self, snap, mask=None):
        """``mask``: as ``VecPushEnv.restore_state`` with N = 1 (a false entry restores nothing)."""
        self._vec.restore_state(snap, mask)
        if getattr(snap, 'host', None) is not None and (mask is None or bool(np.asarray(mask).reshape(-1)[0])):
            self._obs_data, self._prev_obs_data, self._done, self._episode_reward, self._total_reward = snap.host

    def simulate_plans(self, actions):
        """``VecPushEnv.simulate_plans`` for this env: ``actions`` [S, H, G, 4] (or [1, S, H, G, 4]; [S, H, 4] without goal
        steps).  Returns (states [S, H, RV_MAXB, 2], rewards [S, H], dones [S, H])."""
        a = self._vec.world.torch.as_tensor(actions)
        if a.dim() == 2 + len(self._vec.action_shape):
            a = a[None]
        st, r, d = self._vec.simulate_plans(a)
        return st[0], r[0], d[0]

    def sample_plan_candidates(self, mean, std, num_samples, iteration, seed=0, keep_mean=True):
        """``VecPushEnv.sample_plan_candidates`` for this env: ``mean`` / ``std`` [H] + action shape (or with a leading
        1).  Returns [S, H] + action shape."""
        m, s = self._one(mean), self._one(std)
        return self._vec.sample_plan_candidates(m, s, num_samples, iteration, seed, keep_mean)[0]

    def refit_plan_distribution(self, candidates, returns, mean, std, num_elites, alpha=0.0, min_std=0.0):
        """``VecPushEnv.refit_plan_distribution`` for this env: ``candidates`` [S, H] + action shape, ``returns`` [S],
        ``mean`` / ``std`` [H] + action shape (or each with a leading 1).  Returns (mean, std, elite [E])."""
        torch = self._vec.world.torch
        c = torch.as_tensor(candidates)
        if c.dim() == 2 + len(self._vec.action_shape):
            c = c[None]
        r = torch.as_tensor(returns)
        r = r[None] if r.dim() == 1 else r
        m, s, e = self._vec.refit_plan_distribution(c, r, self._one(mean), self._one(std), num_elites, alpha, min_std)
        return m[0], s[0], e[0]

    def sample_heuristic_candidates(self, num_samples, mode='spread', step=0, seed=0, max_attempts=20000,
                                    start_margin=0.05, motion_margin=0.01):
        """``VecPushEnv.sample_heuristic_candidates`` for this env.  Returns (actions [S] + action shape, found [S])."""
        a, f = self._vec.sample_heuristic_candidates(num_samples, mode, step, seed, max_attempts, start_margin, motion_margin)
        return a[0], f[0]

    def propose_plans(self, num_samples, horizon, seed=0, max_attempts=20000, start_margin=0.05, motion_margin=0.01):
        """``VecPushEnv.propose_plans`` for this env.  Returns (actions [S, H] + action shape, states [S, H, RV_MAXB, 2],
        rewards [S, H], dones [S, H], found [S, H])."""
        return tuple(x[0] for x in self._vec.propose_plans(num_samples, horizon, seed, max_attempts, start_margin, motion_margin))

    def sample_route_candidates(self, num_samples, step=0, seed=0, **route):
        """``VecPushEnv.sample_route_candidates`` for this env.  Returns (actions [S] + action shape, found [S])."""
        a, f = self._vec.sample_route_candidates(num_samples, step, seed, **route)
        return a[0], f[0]

    def propose_route_plans(self, num_samples, horizon, seed=0, **route):
        """``VecPushEnv.propose_route_plans`` for this env.  Returns (actions [S, H] + action shape, states [S, H, RV_MAXB,
        2], rewards [S, H], dones [S, H], found [S, H])."""
        return tuple(x[0] for x in self._vec.propose_route_plans(num_samples, horizon, seed, **route))

    def clustered_point_cloud(self, num_points=None, draw_index=0, **overrides):
        """``VecPushEnv.clustered_point_cloud`` for this env (``grouping='ward'`` and ``num_neighbors`` among the
        overrides).  Returns the dict with the leading axis dropped."""
        return {k: v[0] for k, v in self._vec.clustered_point_cloud(num_points, draw_index, **overrides).items()}

    def _one(self, x):
        """[H] + action shape -> [1, H] + action shape"""
        x = self._vec.world.torch.as_tensor(x)
        return x[None] if x.dim() == 1 + len(self._vec.action_shape) else x

    def close(self):
        self._vec.close()
