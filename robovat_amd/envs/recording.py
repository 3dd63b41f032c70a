"""Watching a batched env step: ``record_step`` and the ``RECORDING`` option of PushEnv / Grasp4DofEnv.

The reference's PushEnv has a second camera with its own size and pose, takes a screenshot of it every
``RECORDING.NUM_STEPS`` simulator substeps while an action runs and writes one video per episode (``push_env.py:143-147,
282-327, 657-660, 1155-1162``).  Here an action is one launch, so the pictures are taken of COPIES of the recorded envs:

  the recorded env blocks are copied into a small world (``World.save_state`` / ``load_state``), the copies are given the
  same action with ``step_begin`` and advanced with ``step_poll``, at most ``every`` substeps at a time, and ``render_view``
  draws them after every poll;  the envs themselves then take the action with the plain ``step()``.

``rv_step_poll`` promises that a step cut into launches is the uncut step bit for bit, and a step does not depend on the
env's global id, so the copies go where the envs go: the last frame is the envs' own state after the step (the GPU tests
compare it with a render of the envs).  Polling the envs themselves would give the same trajectory but not the same env
blocks: the per-launch figures (``env_counters()[:, 7:]``, ``stats()``) would be those of the last poll, and the words that
carry a step across a launch boundary (``ms_*``) keep what the last suspension left in them.  With copies the recorded world
computes literally what ``step()`` computes, and the polls cost what the recorded envs cost, not the batch.

A poll is asked for ``every - 1`` substeps: ``rv_step_poll(max_substeps)`` takes ``max_substeps`` or ``max_substeps + 1``
substeps of an env that does not finish (a coasting run that ends on the budget is followed by the regular substep it stopped
at), so two frames are ``every - 1`` or ``every`` substeps apart and never more than ``every``.

Frames are counted from the start of the action -- frame 0 is the state before its first substep, frame t the state at
most t * ``every`` substeps later -- where the reference records whenever ``simulator.num_steps % NUM_STEPS == 0``, a count that
runs on from the reset.  ``sim_steps`` stamps every frame with the env's own counter.
"""
import os

import numpy as np


def _record_world(env, r):
    """the world of ``r`` envs that holds the copies: made on first use and kept per size, same scene, config and seed"""
    worlds = env.__dict__.setdefault('_record_worlds', {})
    w = worlds.get(int(r))
    if w is None:
        from robovat_amd import abi, lib
        cfg = abi.rv_config.from_buffer_copy(bytes(env.rv_config))
        cfg.n_envs = int(r)
        w = worlds[int(r)] = lib.World(cfg, env.scene, device=env.world.device_index)
    return w


def close_record_worlds(env):
    for w in env.__dict__.pop('_record_worlds', {}).values():
        w.close()


def record_step(env, actions, cameras, env_index, every, height=None, width=None, supersample=1, max_frames=256):
    """``env.step(actions)`` with pictures.  ``env``: a VecPushEnv or VecGrasp4DofEnv; ``cameras`` / ``env_index`` /
    ``height`` / ``width`` / ``supersample``: the V views, as ``World.render_view`` takes them (an env may have several);
    ``every`` >= 2: the most substeps between two frames; ``max_frames`` >= 2: the most frames kept.

    Frame 0 is the state before the first substep.  A frame follows every ``every`` - 1 or ``every`` substeps while any recorded env is
    still stepping and fewer than ``max_frames`` - 1 have been taken; after that the step runs to its end unwatched.  The
    last frame is the completed state.  An env that has finished repeats its last image.

    Returns ``(obs, reward, done, info)``: the first three are what ``step(actions)`` returns, bit for bit, and ``info`` --
    None from ``step()`` -- is ``{'frames': uint8 [T, V, H, W, 3] on the device, 'sim_steps': int32 [T, V], the env's
    substep counter (``env_counters()[:, 0]``) at each frame, 'num_frames': T}``."""
    world, torch = env.world, env.world.torch
    every, max_frames = int(every), int(max_frames)
    if every < 2:
        raise ValueError('record_step: every must be at least 2 substeps (a poll may take one more than it is asked for)')
    if max_frames < 2:
        raise ValueError('record_step: max_frames must be at least 2 (the state before and the state after)')
    rows, idx, h, w = world.view_inputs(cameras, env_index, height, width)
    if idx.min() < 0 or idx.max() >= world.n:
        raise ValueError('record_step: env index outside [0, N)')
    uniq, inv = np.unique(idx, return_inverse=True)
    inv = inv.astype(np.int32)
    a = env._world_actions(actions)
    copies = _record_world(env, len(uniq))
    pick = torch.as_tensor(uniq.astype(np.int64), device=world.device)
    copies.load_state(world.save_state(), pick)
    copies.step_begin(a.reshape(world.n, world.G, 4)[pick])
    v = len(idx)
    frames = torch.empty((max_frames, v, h, w, 3), dtype=torch.uint8, device=world.device)
    stamps = torch.empty((max_frames, v), dtype=torch.int32, device=world.device)
    col = torch.as_tensor(inv.astype(np.int64), device=world.device)

    def shoot(t):
        copies.render_view(rows, inv, h, w, supersample, out={'rgb': frames[t]})
        stamps[t] = copies.env_counters()[:, 0][col]

    shoot(0)
    t = 1
    left = torch.ones((len(uniq),), dtype=torch.bool, device=world.device)
    while True:
        watching = t < max_frames - 1
        left &= ~copies.step_poll(max_substeps=every - 1 if watching else 0).bool()
        if not bool(left.any()):
            break
        if watching:
            shoot(t)
            t += 1
    shoot(t)
    t += 1
    obs, reward, done, _ = env._plain_step(actions)
    return obs, reward, done, {'frames': frames[:t], 'sim_steps': stamps[:t], 'num_frames': t}


def camera_of_config(rec):
    """The ``perception.Camera`` of a ``RECORDING.CAMERA`` block: HEIGHT, WIDTH, INTRINSICS (3 x 3), TRANSLATION, ROTATION
    (3 x 3; x_cam = ROTATION x_world + TRANSLATION, as KINECT2.DEPTH)."""
    from robovat_amd.perception import Camera
    c = rec['CAMERA']
    return Camera(height=int(c['HEIGHT']), width=int(c['WIDTH']), intrinsics=np.asarray(c['INTRINSICS'], dtype=np.float64).reshape(3, 3),
                  translation=c['TRANSLATION'], rotation=np.asarray(c['ROTATION'], dtype=np.float64).reshape(3, 3))


class Recorder(object):
    """The ``RECORDING`` option of an env config, with the reference's key names (``push_env.py:143-147, 282-327``):

      USE          False: everything below is ignored (and so is a config without the key)
      CAMERA       {HEIGHT, WIDTH, INTRINSICS, TRANSLATION, ROTATION}: the recording camera
      NUM_STEPS    the most substeps between two frames (at least 2)
      FPS          the rate the files are played at
      OUTPUT_DIR   where the files go, in the subdirectory the reference uses ('data_collection', or '<task>_layoutNN')
      ENVS         ours: the env rows that are recorded (default [0])
      SUPERSAMPLE  ours: rays per pixel and side (default 1)
      FORMAT       ours: 'png' (animated, lossless; the default), 'gif' or 'npz' -- the reference writes XVID .avi through
                   cv2, which is not a dependency here
      MAX_FRAMES   ours: frames kept per action (default 256)

    One file per recorded env and episode, ``env<row>_ep<count>.<format>``: opened by the reset that starts the episode,
    written when that env is reset again or the env object is closed."""

    def __init__(self, env, rec):
        from robovat_amd.io.video_utils import EXTENSIONS
        self.env = env
        self.camera = camera_of_config(rec)
        self.every = int(rec['NUM_STEPS'])
        self.fps = float(rec.get('FPS', 30))
        self.rows = [int(i) for i in rec.get('ENVS', [0])]
        self.supersample = int(rec.get('SUPERSAMPLE', 1))
        self.max_frames = int(rec.get('MAX_FRAMES', 256))
        self.ext = '.' + str(rec.get('FORMAT', 'png')).lower().lstrip('.')
        if self.ext not in EXTENSIONS:
            raise ValueError('RECORDING.FORMAT must be one of %s' % ', '.join(e[1:] for e in EXTENSIONS))
        if self.every < 2 or not self.rows or min(self.rows) < 0 or max(self.rows) >= env.num_envs or len(set(self.rows)) != len(self.rows):
            raise ValueError('RECORDING: NUM_STEPS must be at least 2 and ENVS distinct rows of the %d envs' % env.num_envs)
        task = env.config.get('TASK_NAME')
        sub = 'data_collection' if task is None else '%s_layout%02d' % (task, int(env.config.get('LAYOUT_ID', 0)))
        self.output_dir = os.path.join(str(rec['OUTPUT_DIR']), sub)
        self.writers = {}
        self.episodes = dict((i, 0) for i in self.rows)
        self.paths = []      # the files written so far, in order

    def on_reset(self, mask=None):
        """the reset of the envs flagged in ``mask`` (None: all) ends their files and opens the next ones"""
        from robovat_amd.io.video_utils import FrameWriter
        m = None if mask is None else np.asarray(mask.cpu() if hasattr(mask, 'cpu') else mask).reshape(-1).astype(bool)
        for i in self.rows:
            if m is not None and not m[i]:
                continue
            self._finish(i)
            self.writers[i] = FrameWriter(os.path.join(self.output_dir, 'env%d_ep%04d%s' % (i, self.episodes[i], self.ext)), self.fps)
            self.episodes[i] += 1

    def step(self, actions):
        """``record_step`` of the recorded rows; the frames go to their writers"""
        obs, reward, done, info = record_step(self.env, actions, self.camera, self.rows, self.every,
                                              supersample=self.supersample, max_frames=self.max_frames)
        frames = info['frames'].cpu().numpy()
        for k, i in enumerate(self.rows):
            if i not in self.writers:      # (stepped without a reset: the file starts here)
                self.on_reset(np.arange(self.env.num_envs) == i)
            wr = self.writers[i]
            wr.extend(frames[(1 if len(wr) else 0):, k])      # (frame 0 of a later action is the last frame of the one before)
        return obs, reward, done, None

    def _finish(self, i):
        wr = self.writers.pop(i, None)
        if wr is not None:
            path = wr.close()
            if path:
                self.paths.append(path)

    def close(self):
        for i in list(self.writers):
            self._finish(i)


def make_recorder(env):
    """The Recorder of ``env.config.RECORDING``, or None when the key is missing or USE is false"""
    rec = env.config.get('RECORDING')
    if not rec or not rec.get('USE', False):
        return None
    return Recorder(env, rec)
