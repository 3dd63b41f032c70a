"""Observation classes with the reference's interface (``robovat/observations/*.py``): an
``Observation`` is initialised with the env, exposes ``get_gym_space()`` and
``get_observation()``.  On this backend every observation is a read of device buffers the
kernels fill (``rv_observe`` / ``rv_render`` / ``rv_render_rgb``); the classes below are the
name-compatible handles for code written against the reference.

* ``CameraObs(modality='rgb' | 'depth' | 'segmask')``      camera_obs.py:33-88
* ``SegmentedPointCloudObs``                              camera_obs.py:182-238
* ``PointCloudObs``                                       camera_obs.py:90-124
* ``PoseObs(modality='position' | 'pose' | 'pose2d' | 'yaw_cossin')``   pose_obs.py:17-73
"""
import numpy as np


class _Box(object):
    def __init__(self, low, high, shape, dtype):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype


class Observation(object):
    """observation.py:12-49"""

    def __init__(self, name=None):
        self.name = name
        self.env = None

    def initialize(self, env):
        self.env = env

    def on_episode_start(self):
        pass

    @property
    def world(self):
        return self.env.world


class CameraObs(Observation):
    """Image of the simulated Kinect2 (camera_obs.py:33-88): 'rgb' uint8 [H, W, 3], 'depth' float32
    [H, W, 1] (metres, 0 where nothing is hit), 'segmask' uint8 [H, W, 1] (body index, RV_MAXB + 1 = arm, RV_MAXB =
    table, 255 = nothing).  ``env_index``: which env of a vectorised env (images are per env)."""

    def __init__(self, camera=None, modality='rgb', max_visible_distance_m=None, name=None, env_index=0):
        Observation.__init__(self, name=name or modality)
        if modality not in ('rgb', 'depth', 'segmask'):
            raise ValueError('Unrecognized modality: %r.' % (modality,))
        self.camera, self.modality, self.env_index = camera, modality, int(env_index)
        self.max_visible_distance_m = max_visible_distance_m or 10.0

    def _hw(self):
        c = self.world.cfg
        return int(c.cam_height), int(c.cam_width)

    def get_gym_space(self):
        h, w = self._hw()
        if self.modality == 'rgb':
            return _Box(0, 255, (h, w, 3), np.uint8)
        if self.modality == 'depth':
            return _Box(0.0, self.max_visible_distance_m, (h, w, 1), np.float32)
        return _Box(0, 255, (h, w, 1), np.uint8)

    def get_observation(self):
        i = self.env_index
        if self.modality == 'rgb':
            return self.world.render_rgb()[i].cpu().numpy()
        depth, seg = self.world.render(segmask=True)
        if self.modality == 'depth':
            return depth[i].cpu().numpy()[..., None]
        return seg[i].cpu().numpy()[..., None]


class SegmentedPointCloudObs(Observation):
    """camera_obs.py:182-238: [num_bodies, num_points, 3] per env.  ``segmentation='segmask'`` (the default): grouped by
    the renderer's segmask, from ``rv_observe`` -- the reference's branch with a simulator.  ``segmentation='cluster'``: its
    branch on the real sensor, table plane removed and DBSCAN clusters in the slots (``rv_segment_cloud``, DESIGN.md §25;
    the slots are then in cluster order, not body order); ``segment``: fields of ``lib.segment_params``.  With
    ``grouping='largest'`` (the default) the slots hold the largest DBSCAN clusters and bodies that touch leave one empty;
    ``grouping='ward'`` adds the reference's second ``cluster()`` call, Ward agglomeration of the clustered points on their
    ``num_neighbors``-nearest-neighbour graph into exactly ``num_bodies`` groups (``rv_ward_groups``)."""

    def __init__(self, camera=None, num_points=None, num_bodies=None, crop_min=None, crop_max=None, name=None, env_index=0,
                 segmentation='segmask', draw_index=0, grouping='largest', num_neighbors=100, **segment):
        Observation.__init__(self, name=name or 'point_cloud')
        if segmentation not in ('segmask', 'cluster'):
            raise ValueError('Unrecognized segmentation: %r.' % (segmentation,))
        if grouping not in ('largest', 'ward'):
            raise ValueError('Unrecognized grouping: %r.' % (grouping,))
        self.grouping, self.num_neighbors = grouping, int(num_neighbors)
        self.env_index = int(env_index)
        self.segmentation, self.draw_index, self.segment = segmentation, int(draw_index), dict(segment)
        self.num_points, self.num_bodies = num_points, num_bodies

    def _params(self):
        from robovat_amd import abi, lib
        return lib.segment_params(num_points=int(self.num_points or self.world.cfg.num_points),
                                  num_clusters=int(self.num_bodies or abi.RV_MAXB), draw_index=self.draw_index, **self.segment)

    def get_gym_space(self):
        from robovat_amd import abi
        if self.segmentation == 'cluster':
            p = self._params()
            return _Box(-np.inf, np.inf, (int(p.num_clusters), int(p.num_points), 3), np.float32)
        return _Box(-np.inf, np.inf, (abi.RV_MAXB, int(self.world.cfg.num_points), 3), np.float32)

    def get_observation(self):
        if self.segmentation == 'cluster':
            p = self._params()
            ward = None
            if self.grouping == 'ward':
                from robovat_amd import lib
                ward = lib.ward_params(num_points=int(p.num_points), num_groups=int(p.num_clusters), num_neighbors=self.num_neighbors,
                                       draw_index=self.draw_index)
            return _segment_one(self.world, self.env_index, p, ward)['clouds'][0].cpu().numpy()
        return self.world.observe(point_cloud=True)['point_cloud'][self.env_index].cpu().numpy()


def _segment_one(world, env_index, params, ward=None):
    """render -> deproject -> segment_cloud (-> ward_groups, with ``ward`` params) of one env of the world"""
    depth, _ = world.render(segmask=False)
    pts, valid = world.deproject(depth[env_index:env_index + 1], env_first=env_index)
    r = world.segment_cloud(pts, valid, params, env_first=env_index)
    if ward is not None:
        r = dict(r, **world.ward_groups(pts, r['labels'], ward, env_first=env_index))
    return r


class PointCloudObs(Observation):
    """camera_obs.py:90-124: remove_table -> downsample, [num_points, 3].  The plane stage of ``rv_segment_cloud``, then
    ONE slot that holds every survivor: eps is set so large (1e15 m) that all survivors are neighbours, min_samples 1.  More
    than RV_SEG_MAXPTS survivors are thinned to that many evenly spaced ones before the draw."""
    ALL_EPS = 1e15

    def __init__(self, camera=None, num_points=None, crop_min=None, crop_max=None, name=None, env_index=0, draw_index=0,
                 plane_thresh=0.015, num_hypotheses=50):
        Observation.__init__(self, name=name or 'point_cloud')
        self.env_index, self.draw_index, self.num_points = int(env_index), int(draw_index), num_points
        self.plane_thresh, self.num_hypotheses = float(plane_thresh), int(num_hypotheses)

    def _params(self):
        from robovat_amd import lib
        return lib.segment_params(num_points=int(self.num_points or self.world.cfg.num_points), num_clusters=1,
                                  draw_index=self.draw_index, eps=self.ALL_EPS, min_samples=1, plane_thresh=self.plane_thresh,
                                  num_hypotheses=self.num_hypotheses)

    def get_gym_space(self):
        return _Box(-np.inf, np.inf, (int(self._params().num_points), 3), np.float32)

    def get_observation(self):
        return _segment_one(self.world, self.env_index, self._params())['clouds'][0, 0].cpu().numpy()


class PoseObs(Observation):
    """pose_obs.py:17-73."""

    def __init__(self, num_bodies=None, modality='position', name=None, env_index=0):
        Observation.__init__(self, name=name or modality)
        if modality not in ('position', 'pose', 'pose2d', 'yaw_cossin'):
            raise ValueError('Unrecognized modality: %r.' % (modality,))
        self.modality, self.env_index = modality, int(env_index)

    def get_gym_space(self):
        from robovat_amd import abi
        k = {'position': 3, 'pose': 6, 'pose2d': 3, 'yaw_cossin': 2}[self.modality]
        return _Box(-np.inf, np.inf, (abi.RV_MAXB, k), np.float32)

    def get_observation(self):
        return self.world.observe(pose_modes=True)[self.modality][self.env_index].cpu().numpy()
