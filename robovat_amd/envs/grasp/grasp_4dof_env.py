"""Grasp4DofEnv on the MI355X backend (BASELINE.json configs[3]).

``VecGrasp4DofEnv``: N envs, ``step(actions)`` is one ``rv_step_macro`` launch running the whole
``_execute_action`` phase machine (overhead -> prestart -> straight-line descent -> close -> lift;
``robovat/envs/grasp/grasp_4dof_env.py:213-345``) with the force-limited gripper in the contact
solver, the depth observation and ``GraspReward`` (``reward_fns/grasp_reward.py:49-68``).
``Grasp4DofEnv`` keeps the reference's single-env API as a batch of one.  Actions are
``[x, y, z, angle]`` in the world (``ACTION.TYPE == 'CUBOID'``) or ``[x1, y1, x2, y2, depth]`` in
the depth image (``'IMAGE'``, converted on the host by ``Grasp2D``).
"""
import collections

import numpy as np

from robovat_amd import abi, configs, scenes
from robovat_amd.envs.grasp.grasp_2d import Grasp2D
from robovat_amd.envs.push.push_env import Box
from robovat_amd.perception import Camera


class VecGrasp4DofEnv(object):

    def __init__(self, num_envs, config=None, robot_config=None, device=0, seed=0, env_id_offset=0):
        from robovat_amd import lib
        self.config = config or configs.grasp_env_config()
        self.robot_config = robot_config or configs.sawyer_config()
        self.scene, self.shape_names = scenes.make_scene(env_cfg=self.config)
        self.rv_config = configs.make_rv_config(self.config, self.robot_config, self.shape_names,
                                                n_envs=num_envs, env_id_offset=env_id_offset, seed=seed)
        self.world = lib.World(self.rv_config, self.scene, device=device)
        self.num_envs = int(num_envs)
        c = self.rv_config
        fx, fy, cx, cy, sk = list(c.cam_intrinsics)
        self.camera = Camera(height=c.cam_height, width=c.cam_width, intrinsics=[[fx, sk, cx], [0, fy, cy], [0, 0, 1]],
                             translation=list(c.cam_translation), rotation=np.array(list(c.cam_rotation)).reshape(3, 3))
        if self.config.ACTION.TYPE == 'CUBOID':
            self.action_space = Box(np.array(list(self.config.ACTION.CUBOID.LOW) + [0.0], np.float32),
                                    np.array(list(self.config.ACTION.CUBOID.HIGH) + [2 * np.pi], np.float32))
        elif self.config.ACTION.TYPE == 'IMAGE':
            w, h = c.cam_width, c.cam_height
            self.action_space = Box(np.array([0, 0, 0, 0, -(2 * 24 - 1)], np.float32), np.array([w, h, w, h, 2 * 24 - 1], np.float32))
        else:
            raise ValueError('Unrecognized action type: %r' % (self.config.ACTION.TYPE,))
        self._macro_index = 0
        self.antipodal_status = self.antipodal_image_grasps = None
        self.antipodal_count = self.antipodal_actions4 = None
        self.refine_parent = None
        self._plan_worlds = {}
        from robovat_amd.envs import recording
        self._recorder = recording.make_recorder(self)      # config.RECORDING (None: off, the default)

    device = property(lambda s: s.world.device)

    def get_observation(self):
        """CameraObs(OBSERVATION.TYPE = 'depth') + the camera calibration (grasp_4dof_env.py:97-115).

        With ``OBSERVATION.DEPTH_NOISE`` set ({GAMMA_SHAPE, PROB, RESCALE_FACTOR, SIGMA, SEED}) the depth carries the
        sensor noise of ``rv_depth_noise``, drawn with ``draw_index`` = the number of ``step()`` calls so far: the
        observation of ``reset()`` on a fresh env uses index 0, the one ``step()`` k returns uses k >= 1 (a later
        ``reset()`` uses the count at that moment, the step after it the next one), and asking again between two steps
        returns the same noise.  None (the default): the render as it is, nothing launched.
        ``sample_antipodal_*(depth=None)`` render a clean image of their own whatever this says; a policy that is handed
        this observation's depth sees the noise."""
        depth, _ = self.world.render()
        noise = self.config['OBSERVATION'].get('DEPTH_NOISE')
        if noise is not None:
            from robovat_amd import lib
            depth = self.world.depth_noise(depth, lib.depth_noise_params(noise, draw_index=self._macro_index), out=depth)
        k, t, r = self.camera_calibration()
        return {'depth': depth, 'intrinsics': k, 'translation': t, 'rotation': r}

    def camera_calibration(self):
        """(intrinsics [N, 3, 3], translation [N, 3], rotation [N, 3, 3]) each env is rendered with: the configured
        calibration plus the noise of its last reset (ArmEnv._reset_camera, arm_env.py:109-152; rv_get_camera)."""
        cam = self.world.camera().cpu().numpy()
        k = np.zeros((self.num_envs, 3, 3), np.float32)
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2], k[:, 0, 1], k[:, 2, 2] = cam[:, 0], cam[:, 1], cam[:, 2], cam[:, 3], cam[:, 4], 1.0
        return k, cam[:, 14:17].copy(), cam[:, 5:14].reshape(-1, 3, 3).copy()

    def reset(self, mask=None):
        self.world.reset(mask)
        if self._recorder is not None:
            self._recorder.on_reset(mask)
        return self.get_observation()

    def _to_4dof(self, actions):
        if self.config.ACTION.TYPE == 'CUBOID':
            return actions
        a = np.asarray(actions.cpu() if hasattr(actions, 'cpu') else actions, np.float64).reshape(self.num_envs, 5)
        return np.array([Grasp2D.from_vector(v, camera=self.camera).as_4dof() for v in a], np.float32)

    def step(self, actions):
        """With ``config.RECORDING.USE`` the step goes through ``record_step`` and the frames of the recorded envs go to
        their episode files (``envs/recording.py``)."""
        if self._recorder is not None:
            return self._recorder.step(actions)
        return self._plain_step(actions)

    def _world_actions(self, actions):
        """the actions as the world takes them: float32 [N, 1, 4] on the device"""
        return self.world._in(self._to_4dof(actions), (self.num_envs, self.world.G, 4), self.world.torch.float32)

    def record_step(self, actions, cameras, env_index, every, height=None, width=None, supersample=1, max_frames=256):
        """``step(actions)`` watched through free cameras (``envs.recording.record_step``): returns (obs, reward, done,
        {'frames' uint8 [T, V, H, W, 3], 'sim_steps' int32 [T, V], 'num_frames'}) -- a frame of every view before the first
        substep, then at most ``every`` (>= 2) substeps apart, and of the completed state.  The first three are ``step()``'s bit for bit."""
        from robovat_amd.envs import recording
        return recording.record_step(self, actions, cameras, env_index, every, height, width, supersample, max_frames)

    def _plain_step(self, actions):
        self.world.set_actions(self._to_4dof(actions))
        self.world.step_macro()
        self._macro_index += 1
        obs = self.get_observation()
        reward, done = self.world.reward()
        return obs, reward, done.bool(), None

    def sample_random_actions(self):
        """RandomPolicy = action_space.sample() on the device (uniform in ACTION.CUBOID x [0, 2 pi))."""
        return self.world.policy_random(self._macro_index).reshape(self.num_envs, 4)

    def sample_antipodal_actions(self, depth=None, config=None):
        """AntipodalGrasp4DofPolicy on the device (rv_policy_antipodal): one antipodal grasp per env from its depth
        image (``depth`` [N, H, W]; None: rendered now), in the env's ACTION.TYPE -- [N, 4] world actions for
        'CUBOID', [N, 5] image grasps for 'IMAGE'.  Rows without a grasp carry the env's RandomPolicy draw (see
        ``antipodal_status``: 1 = grasp; 0 / -1 / -2 / -3 = no edge pixel / no valid pair / every candidate rejected /
        too many edge pixels); the status and the image grasps stay on the env for recording."""
        from robovat_amd import lib
        cuboid = self.config.ACTION.TYPE == 'CUBOID'
        g, a, st = self.world.policy_antipodal(lib.antipodal_params(config), self._macro_index, depth=depth, actions4=cuboid)
        self.antipodal_status, self.antipodal_image_grasps = st, g
        return a if cuboid else g

    def sample_antipodal_candidates(self, num_samples, depth=None, config=None):
        """The reference sampler's ``sample(depth, camera, num_samples)`` on the device (rv_policy_antipodal_multi): up
        to ``num_samples`` (K <= abi.RV_AP_MAX_SAMPLES) distinct antipodal grasps per env, in the env's ACTION.TYPE --
        [N, K, 4] world actions for 'CUBOID', [N, K, 5] image grasps for 'IMAGE'.  Candidate 0 is the grasp
        ``sample_antipodal_actions`` returns; ``antipodal_count`` [N] says how many an env found, the rows from there
        on repeat candidate 0, and an env without any (``antipodal_status`` != 1) carries its RandomPolicy draw in all K
        rows.  ``antipodal_status``, ``antipodal_count``, ``antipodal_image_grasps`` [N, K, 5] and
        ``antipodal_actions4`` [N, K, 4] (the env's own calibration; what ``try_grasps`` takes) stay on the env."""
        from robovat_amd import lib
        g, a, cnt, st = self.world.policy_antipodal_multi(lib.antipodal_params(config), self._macro_index, num_samples,
                                                          depth=depth, actions4=True)
        self.antipodal_status, self.antipodal_count = st, cnt
        self.antipodal_image_grasps, self.antipodal_actions4 = g, a
        return a if self.config.ACTION.TYPE == 'CUBOID' else g

    def grasp_images(self, image_grasps=None, depth=None, **crop):
        """The input of a grasp-quality model for every candidate (rv_grasp_crops): the depth image
        re-centred on the grasp, rotated so that the grasp axis is horizontal, and cropped.  ``image_grasps`` [N, K, 5] or
        [N, 5] (None: ``antipodal_image_grasps`` of the last sampling call; ValueError if there was none); ``depth``
        [N, H, W] (None: rendered now, without sensor noise); ``crop``: the fields of ``lib.grasp_crop_params``.
        Returns (images float32 [N, K, h, w], grasp depths float32 [N, K]) on the device."""
        from robovat_amd import lib
        if image_grasps is None:
            image_grasps = self.antipodal_image_grasps
            if image_grasps is None:
                raise ValueError('grasp_images: no image grasps given and no antipodal sampling call before this one')
        if depth is None:
            depth, _ = self.world.render()
        return self.world.grasp_crops(depth, image_grasps, lib.grasp_crop_params(**crop))

    def grasp_qualities(self, model, image_grasps=None, depth=None, **crop):
        """The logits of a grasp-quality model for every candidate (rv_grasp_quality): ``grasp_images`` with
        the model's height x width (``crop`` may give ``step``, default 3), then ``World.grasp_quality``.  ``model``: a
        ``perception.grasp_quality.GraspQualityModel``; ``image_grasps`` and ``depth`` as in ``grasp_images`` (None: the
        last sampling call's grasps, a render made now).  Returns float32 [N, K] on the device; the envs do not change."""
        crop = dict(crop, crop_height=model.sizes['height'], crop_width=model.sizes['width'])
        images, grasp_depths = self.grasp_images(image_grasps, depth, **crop)
        return self.world.grasp_quality(images, grasp_depths, model)

    def refine_grasps(self, scores, num_elites, sigmas, iteration, image_grasps=None, depth=None, config=None, seed=0):
        """One cross-entropy step on the candidates (rv_grasp_refine), one launch: the K rows of
        ``antipodal_image_grasps`` are ranked per env by ``scores`` [N, K] (logits of ``grasp_qualities``, rewards of
        ``try_grasps``, ...), the best ``num_elites`` stay -- in rank order, bit for bit, so row 0 is the best candidate --
        and every other row becomes a child of an elite: centre, axis angle and depth perturbed by normals of ``sigmas`` =
        (pixels, radians, metres), kept when it passes the sampler's boundary and depth-window checks of ``config`` (an
        AntipodalGrasp4DofPolicy config; None: the default), else its parent again.  ``iteration``: the refinement round,
        part of the Philox key with the env's next step index and ``seed``.  ``depth`` [N, H, W] (None: rendered now,
        without sensor noise).  ``image_grasps`` None: the last sampling or refinement call's rows with their
        ``antipodal_count`` / ``antipodal_status`` (ValueError if there was none); given: [N, K, 5], every row a candidate.
        Replaces ``antipodal_image_grasps``, ``antipodal_actions4`` and ``antipodal_count`` (K, or 0 for an env without a
        candidate, whose rows stay as they are); keeps ``refine_parent`` int32 [N, K]: the input row of each output row,
        -1 - row for a child that fell back to its parent.  Returns the new candidates in the env's ACTION.TYPE."""
        from robovat_amd import lib
        count = status = None
        if image_grasps is None:
            image_grasps, count, status = self.antipodal_image_grasps, self.antipodal_count, self.antipodal_status
            if image_grasps is None or image_grasps.dim() != 3:
                raise ValueError('refine_grasps: no image grasps given and no sample_antipodal_candidates call before this one')
        if depth is None:
            depth, _ = self.world.render()
        sc, sa, sd = [float(v) for v in sigmas]
        params = lib.grasp_refine_params(n_elites=num_elites, sigma_center=sc, sigma_angle=sa, sigma_depth=sd,
                                         macro_index=self._macro_index, iteration=iteration, seed=seed)
        g, a, parent, cnt = self.world.grasp_refine(depth, image_grasps, scores, params, lib.antipodal_params(config),
                                                    count=count, status=status, actions4=True)
        self.antipodal_image_grasps, self.antipodal_actions4, self.antipodal_count = g, a, cnt
        self.refine_parent = parent
        return a if self.config.ACTION.TYPE == 'CUBOID' else g

    def collect_grasp_samples(self, num_samples, depth=None, config=None, **crop):
        """Labelled grasp samples of the envs as they are now: one depth image (``depth`` [N, H, W]; None: rendered once,
        without sensor noise) goes to ``sample_antipodal_candidates(num_samples)`` and to ``grasp_images``, then
        ``try_grasps(antipodal_actions4)`` executes every candidate on a copy of its env.  The envs themselves do not
        change.  Returns a dict of device tensors: ``images`` [N, K, h, w], ``grasp_depths`` [N, K], ``image_grasps``
        [N, K, 5], ``actions4`` [N, K, 4], ``rewards`` [N, K], ``dones`` uint8 [N, K], ``count`` int32 [N], ``status``
        int32 [N] and ``valid`` bool [N, K] = status[n] == 1 and k < count[n].  Rows from ``count`` on repeat row 0 and an
        env without a grasp carries its RandomPolicy draw: ``valid`` is how a consumer leaves them out."""
        torch = self.world.torch
        if depth is None:
            depth, _ = self.world.render()
        self.sample_antipodal_candidates(num_samples, depth=depth, config=config)
        grasps, actions4 = self.antipodal_image_grasps, self.antipodal_actions4
        count, status = self.antipodal_count, self.antipodal_status
        images, grasp_depths = self.grasp_images(grasps, depth, **crop)
        rewards, dones = self.try_grasps(actions4)
        k = torch.arange(int(grasps.shape[1]), device=self.device, dtype=torch.int32)
        valid = (status == 1)[:, None] & (k[None, :] < count[:, None])
        return {'images': images, 'grasp_depths': grasp_depths, 'image_grasps': grasps, 'actions4': actions4,
                'rewards': rewards, 'dones': dones, 'count': count, 'status': status, 'valid': valid}

    def save_state(self):
        """All N envs as they are now (``lib.World.save_state``): a ``lib.Snapshot`` on the device, plus the index of the
        env's next policy draw."""
        snap = self.world.save_state()
        snap.macro_index = self._macro_index
        return snap

    def restore_state(self, snap, mask=None):
        """Put the envs back where ``snap`` was taken: all of them, or those flagged in ``mask`` (bool [N]; the others
        keep their present state).  From then on they continue bit for bit as they did after the snapshot."""
        if mask is None:
            self.world.load_state(snap)
            if getattr(snap, 'macro_index', None) is not None:
                self._macro_index = snap.macro_index
            return
        torch = self.world.torch
        m = torch.as_tensor(mask, device=self.device).reshape(self.num_envs).bool()
        ar = torch.arange(self.num_envs, device=self.device, dtype=torch.int32)
        self.world.load_state(snap, torch.where(m, ar, torch.full_like(ar, -1)))

    def _plan_world(self, k):
        """the world of N x K envs behind try_grasps: made on first use and kept per K; same scene, config and seed"""
        w = self._plan_worlds.get(int(k))
        if w is None:
            from robovat_amd import lib
            cfg = abi.rv_config.from_buffer_copy(bytes(self.rv_config))
            cfg.n_envs = self.num_envs * int(k)
            cfg.env_id_offset = int(self.rv_config.env_id_offset) * int(k)
            w = self._plan_worlds[int(k)] = lib.World(cfg, self.scene, device=self.world.device_index)
        return w

    def try_grasps(self, actions4):
        """Look ahead with the simulator: ``actions4`` [N, K, 4] are K candidate world actions [x, y, z, angle] per env
        (``antipodal_actions4``).  Each is executed on a bit-exact copy of its env -- env j * K + k of a world of N x K
        envs becomes env j (rv_branch) and takes one env.step() with candidate k -- and the envs themselves do not
        change.  Returns (rewards float32 [N, K], dones uint8 [N, K]): what ``step`` would return for that action."""
        torch = self.world.torch
        a = torch.as_tensor(actions4, dtype=torch.float32, device=self.device)
        if a.dim() != 3 or int(a.shape[0]) != self.num_envs or int(a.shape[1]) < 1 or int(a.shape[2]) != 4:
            raise ValueError('try_grasps: actions4 must be [N, K, 4] with N = %d, got %s' % (self.num_envs, tuple(a.shape)))
        k = int(a.shape[1])
        w = self._plan_world(k)
        w.branch_from(self.world, k)
        w.set_actions(a.reshape(self.num_envs * k, 4))
        w.step_macro()
        r, d = w.reward()
        return r.reshape(self.num_envs, k), d.reshape(self.num_envs, k)

    def contact_points(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1, capacity=abi.RV_CP_MAX):
        """PyBullet contact records of every env on the device (``lib.World.contact_points``): ids [N, P, 4],
        data [N, P, RV_CP_NF], count [N]; bodies are slots, ``abi.RV_CP_TABLE`` or ``abi.RV_CP_ARM``."""
        return self.world.contact_points(body_a, link_a, body_b, link_b, capacity)

    def contact_forces(self, body_a=-1, link_a=-1, body_b=-1, link_b=-1):
        """Net contact force on body A, [N, 3] on the device (``lib.World.contact_forces``)."""
        return self.world.contact_forces(body_a, link_a, body_b, link_b)

    def rollout(self, n_steps, auto_reset=True, record=True):
        out = self.world.rollout(n_steps, self._macro_index, auto_reset, record)
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
        self.world.close()


class Grasp4DofEnv(object):
    """Single-env Grasp4DofEnv with the reference's API (a VecGrasp4DofEnv of one)."""

    def __init__(self, simulator=None, config=None, debug=False, robot_config=None, device=0, seed=0, worker_id=0):
        self._config = config or configs.grasp_env_config()
        self._debug, self._simulator = debug, simulator
        self._vec = VecGrasp4DofEnv(1, self._config, robot_config, device=device, seed=seed, env_id_offset=worker_id)
        self.camera = self._vec.camera
        self.action_space = self._vec.action_space
        self._obs_data = None
        self._done = True
        self._episode_reward = self._total_reward = 0.0

    config = property(lambda s: s._config)
    debug = property(lambda s: s._debug)
    simulator = property(lambda s: s._simulator)
    is_simulation = property(lambda s: True)
    done = property(lambda s: s._done)
    episode_reward = property(lambda s: s._episode_reward)
    total_reward = property(lambda s: s._total_reward)
    obs_data = property(lambda s: s._obs_data)
    num_steps = property(lambda s: int(s._vec.world.env_counters().cpu().numpy()[0, 1]))
    num_episodes = property(lambda s: int(s._vec.world.env_counters().cpu().numpy()[0, 2]))

    def _convert(self, obs):
        out = collections.OrderedDict()
        out[self._config.OBSERVATION.TYPE] = obs['depth'][0].cpu().numpy()
        for key in ('intrinsics', 'translation', 'rotation'):
            out[key] = obs[key][0]
        return out

    def reset(self):
        self._obs_data = self._convert(self._vec.reset())
        self._done = False
        self._episode_reward = 0.0
        return self._obs_data

    def step(self, action):
        if self._done:
            raise ValueError('The environment is done. Forget to reset?')
        n = 4 if self._config.ACTION.TYPE == 'CUBOID' else 5
        return self._took(self._vec.step(np.asarray(action, np.float32).reshape(1, n)))

    def _took(self, out):
        """the bookkeeping of one step of the batch of one; the fourth entry is passed through"""
        obs, reward, done, info = out
        self._obs_data = self._convert(obs)
        reward = float(reward[0].item())
        self._done = bool(done[0].item())
        self._episode_reward += reward
        if self._done:
            self._total_reward += self._episode_reward
        return self._obs_data, reward, self._done, info

    def record_step(self, action, cameras, every, height=None, width=None, supersample=1, max_frames=256):
        """``step(action)`` watched through ``cameras`` (``VecGrasp4DofEnv.record_step`` for this env): the fourth entry is
        {'frames' uint8 [T, V, H, W, 3], 'sim_steps' int32 [T, V], 'num_frames'}."""
        if self._done:
            raise ValueError('The environment is done. Forget to reset?')
        n = 4 if self._config.ACTION.TYPE == 'CUBOID' else 5
        return self._took(self._vec.record_step(np.asarray(action, np.float32).reshape(1, n), cameras, [0], every, height, width,
                                                supersample, max_frames))

    def get_observation(self):
        return self._obs_data

    def sample_antipodal_actions(self, depth=None, config=None):
        """AntipodalGrasp4DofPolicy's action for this env (the batch of one); ValueError when no grasp is found, as
        the reference's sampler raises or returns none (image_grasp_sampler.py:359-360)."""
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        a = self._vec.sample_antipodal_actions(depth, config)
        status = int(self._vec.antipodal_status[0].item())
        if status != 1:
            raise ValueError('Failed to sample any valid grasp (antipodal status %d).' % status)
        return a[0].cpu().numpy()

    def sample_antipodal_candidates(self, num_samples, depth=None, config=None):
        """Up to ``num_samples`` antipodal grasps for this env, [K, 4] or [K, 5] by ACTION.TYPE (rows past the number
        found, ``antipodal_count``, repeat the first); ValueError when none is found."""
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        a = self._vec.sample_antipodal_candidates(num_samples, depth, config)
        status = int(self._vec.antipodal_status[0].item())
        if status != 1:
            raise ValueError('Failed to sample any valid grasp (antipodal status %d).' % status)
        return a[0].cpu().numpy()

    def grasp_images(self, image_grasps=None, depth=None, **crop):
        """Grasp-centred depth crops of this env's image: ``image_grasps`` [K, 5] or [5] (None: those of the last
        sampling call; ValueError if there was none), ``depth`` [H, W] (None: rendered now).  Returns NumPy (images
        [K, h, w], grasp depths [K])."""
        if image_grasps is not None:
            image_grasps = np.asarray(image_grasps, np.float32).reshape(1, -1, 5)
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        images, depths = self._vec.grasp_images(image_grasps, depth, **crop)
        return images[0].cpu().numpy(), depths[0].cpu().numpy()

    def grasp_qualities(self, model, image_grasps=None, depth=None, **crop):
        """``VecGrasp4DofEnv.grasp_qualities`` for this env: ``image_grasps`` [K, 5] or [5] (None: those of the last
        sampling call), ``depth`` [H, W] (None: rendered now).  Returns NumPy logits [K]."""
        if image_grasps is not None:
            image_grasps = np.asarray(image_grasps, np.float32).reshape(1, -1, 5)
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        return self._vec.grasp_qualities(model, image_grasps, depth, **crop)[0].cpu().numpy()

    def collect_grasp_samples(self, num_samples, depth=None, config=None, **crop):
        """``VecGrasp4DofEnv.collect_grasp_samples`` for this env: the same dict as NumPy arrays without the env axis
        (``images`` [K, h, w], ..., ``count`` and ``status`` scalars, ``valid`` [K]).  An env without a grasp is not an
        error here: its ``valid`` is all False."""
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        out = self._vec.collect_grasp_samples(num_samples, depth, config, **crop)
        return {key: v[0].cpu().numpy() for key, v in out.items()}

    def refine_grasps(self, scores, num_elites, sigmas, iteration, image_grasps=None, depth=None, config=None, seed=0):
        """``VecGrasp4DofEnv.refine_grasps`` for this env: ``scores`` [K], ``image_grasps`` [K, 5] (None: those of the last
        sampling or refinement call), ``depth`` [H, W] (None: rendered now).  Returns NumPy [K, 4] or [K, 5] by ACTION.TYPE."""
        if image_grasps is not None:
            image_grasps = np.asarray(image_grasps, np.float32).reshape(1, -1, 5)
        if depth is not None:
            depth = np.asarray(depth, np.float32).reshape((1,) + np.shape(depth)[-2:])
        if not hasattr(scores, 'dim'):
            scores = np.asarray(scores, np.float32)
        out = self._vec.refine_grasps(scores.reshape(1, -1), num_elites, sigmas, iteration, image_grasps, depth, config, seed)
        return out[0].cpu().numpy()

    antipodal_status = property(lambda s: s._vec.antipodal_status)
    antipodal_count = property(lambda s: s._vec.antipodal_count)
    antipodal_image_grasps = property(lambda s: s._vec.antipodal_image_grasps)
    antipodal_actions4 = property(lambda s: s._vec.antipodal_actions4)
    refine_parent = property(lambda s: s._vec.refine_parent)

    def save_state(self):
        return self._vec.save_state()

    def restore_state(self, snap, mask=None):
        self._vec.restore_state(snap, mask)

    def try_grasps(self, actions4):
        """``actions4`` [K, 4]: (rewards float32 [K], dones uint8 [K]) of each tried on a copy of this env."""
        r, d = self._vec.try_grasps(np.asarray(actions4, np.float32).reshape(1, -1, 4))
        return r[0].cpu().numpy(), d[0].cpu().numpy()

    def close(self):
        self._vec.close()
