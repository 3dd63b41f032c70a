"""rv_deproject / rv_segment_cloud on the device: bit for bit equal to the NumPy restatement
(tests/segment_host.py) on the clouds scikit-learn labelled, the plane, grouping and overflow clouds and the push world's
own render, with guard words around every output; every refusal; the chunked env method, the observation classes, and the
purity of the clusters of the device's render."""
import ctypes as C

import numpy as np
import pytest

import segment_cases as sc
import segment_host as sh
from robovat_amd import abi, lib

pytestmark = pytest.mark.gpu
GUARD = 64
GOLDEN, _ = sc.golden()
OFFSET = 5


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def world():
    cfg, scene = sc.push_crop_cfg(4, env_id_offset=OFFSET)
    w = lib.World(cfg, scene, device=0)
    w.reset()
    yield w
    w.close()


def _guarded(w, shape, dtype, fill):
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=w.device)
    return buf, buf[GUARD:GUARD + n].view(shape)


def run(w, points, valid, p, env_first=0):
    """rv_segment_cloud with guard words on both sides of every output -> dict of NumPy arrays"""
    import torch
    pts = torch.as_tensor(np.ascontiguousarray(points, np.float32), device=w.device)
    v = None if valid is None else torch.as_tensor(np.ascontiguousarray(valid, np.uint8), device=w.device)
    n, m = pts.shape[0], pts.shape[1]
    par = lib.segment_params(**p)
    c, q = int(par.num_clusters), int(par.num_points)
    specs = dict(labels=((n, m), torch.int32, 0x5A5A5A5), clouds=((n, c, q, 3), torch.float32, -77.0),
                 slot_labels=((n, c), torch.int32, 0x5A5A5A5), slot_counts=((n, c), torch.int32, 0x5A5A5A5),
                 plane=((n, 4), torch.float32, -77.0), info=((n, 8), torch.int32, 0x5A5A5A5))
    bufs = {k: _guarded(w, *s) for k, s in specs.items()}
    ptr = {k: C.c_void_p(b[1].data_ptr()) for k, b in bufs.items()}
    lib.check(w.lib.rv_segment_cloud(w.h, C.byref(par), int(env_first), n, C.c_void_p(pts.data_ptr()), None if v is None else C.c_void_p(v.data_ptr()),
                                     m, ptr['labels'], ptr['clouds'], ptr['slot_labels'], ptr['slot_counts'], ptr['plane'], ptr['info']))
    w.synchronize()
    out = {}
    for k, (buf, view) in bufs.items():
        fill = specs[k][2]
        g = _np(buf)
        assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), 'guard words of %s' % k
        out[k] = _np(view).copy()
    return out


def same(got, want, who=''):
    for k in ('labels', 'slot_labels', 'slot_counts', 'info'):
        assert np.array_equal(got[k], want[k]), (who, k, got[k], want[k])
    for k in ('clouds', 'plane'):
        assert np.array_equal(got[k].view(np.uint32), np.ascontiguousarray(want[k], np.float32).view(np.uint32)), (who, k)


def pad(clouds, masks):
    """clouds of different sizes as one [n, M, 3] batch, the padding masked out"""
    m = max(len(c) for c in clouds)
    pts = np.full((len(clouds), m, 3), np.nan, np.float32)
    valid = np.zeros((len(clouds), m), np.uint8)
    for e, (c, v) in enumerate(zip(clouds, masks)):
        pts[e, :len(c)] = c
        valid[e, :len(c)] = 1 if v is None else v
    return pts, valid


@pytest.mark.parametrize('k', range(len(GOLDEN)), ids=[c['name'] for c in GOLDEN])
def test_golden_clouds(world, k):
    """three different clouds in one call (envs 1 .. 3 of the world); env 0 of the call is case k with its own
    min_samples, so its labels are scikit-learn's too"""
    cases = [GOLDEN[(k + j) % len(GOLDEN)] for j in range(3)]
    pts, valid = pad([c['points'] for c in cases], [c['valid'] for c in cases])
    p = sc.params(num_hypotheses=0, min_samples=cases[0]['min_samples'], num_clusters=3, num_points=33)
    got = run(world, pts, valid, p, env_first=1)
    want = sh.segment_batch(pts, valid, p, sc.world_seed(world.cfg), OFFSET + 1)
    same(got, want, cases[0]['name'])
    assert np.array_equal(got['labels'][0][valid[0] != 0], cases[0]['labels'])
    assert not (got['info'][:, abi.RV_SEG_INFO_FLAGS] & abi.RV_SEG_FLAG_BOUND).any()
    # with a plane stage on the same clouds (whatever it removes, the same on both sides)
    p2 = dict(p, num_hypotheses=16, plane_thresh=0.004)
    same(run(world, pts, valid, p2, env_first=1), sh.segment_batch(pts, valid, p2, sc.world_seed(world.cfg), OFFSET + 1), 'with plane')


def test_plane_cloud(world):
    pts, dist = sc.plane_cloud()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.001]], np.float32)
    batch, valid = pad([pts, tri[:3], tri, tri[:2]], [None] * 4)
    for p in (sc.params(min_samples=20, num_clusters=2, num_points=64), sc.params(num_hypotheses=64, min_samples=1, num_points=5),
              sc.params(num_hypotheses=1024, min_samples=20, num_points=7, draw_index=(1 << 32) - 1)):
        got = run(world, batch, valid, p)
        same(got, sh.segment_batch(batch, valid, p, sc.world_seed(world.cfg), OFFSET), 'plane')
    got = run(world, batch, valid, sc.params(min_samples=20, num_clusters=2, num_points=64))
    assert np.array_equal(got['labels'][0] == abi.RV_SEG_PLANE, np.abs(dist) <= sc.THRESH)
    assert got['info'][3, abi.RV_SEG_INFO_FLAGS] & abi.RV_SEG_FLAG_NO_PLANE and got['info'][3, abi.RV_SEG_INFO_BEST_H] == -1
    # without a mask, with a NaN and an infinity among the points
    bad = pts.copy(); bad[5, 1] = np.nan; bad[9, 2] = np.inf
    p = sc.params(min_samples=20, num_clusters=2, num_points=64)
    got = run(world, bad[None], None, p, env_first=3)
    same(got, sh.segment_batch(bad[None], None, p, sc.world_seed(world.cfg), OFFSET + 3), 'non-finite')
    assert got['labels'][0, 5] == abi.RV_SEG_INVALID and got['labels'][0, 9] == abi.RV_SEG_INVALID


@pytest.mark.parametrize('P', [1, 64, 65])
def test_grouping_cloud(world, P):
    pts, lab = sc.grouping_cloud()
    for c, draw in ((8, 0), (2, 0), (8, 7), (16, 3)):
        p = sc.params(num_hypotheses=0, min_samples=5, num_clusters=c, num_points=P, draw_index=draw)
        got = run(world, np.stack([pts, pts[::-1]]), None, p, env_first=2)
        same(got, sh.segment_batch(np.stack([pts, pts[::-1]]), None, p, sc.world_seed(world.cfg), OFFSET + 2), 'grouping')
        assert np.array_equal(got['labels'][0], lab)


def test_overflow_cloud(world):
    pts = sc.overflow_cloud()
    p = sc.params(num_hypotheses=0, num_points=300)
    got = run(world, pts[None], None, p)
    same(got, sh.segment_batch(pts[None], None, p, sc.world_seed(world.cfg), OFFSET), 'overflow')
    assert got['info'][0, abi.RV_SEG_INFO_KEPT] == abi.RV_SEG_MAXPTS and got['info'][0, abi.RV_SEG_INFO_FLAGS] & abi.RV_SEG_FLAG_OVERFLOW
    assert (got['labels'][0] == abi.RV_SEG_SKIPPED).sum() == 9000 - abi.RV_SEG_MAXPTS
    # one slot that holds everything, as PointCloudObs asks for it: every point a neighbour of every other
    p = sc.params(num_hypotheses=0, eps=1e15, min_samples=1, num_clusters=1, num_points=256)
    got = run(world, pts[None, :2500], None, p)
    same(got, sh.segment_batch(pts[None, :2500], None, p, sc.world_seed(world.cfg), OFFSET), 'one slot')
    assert got['slot_counts'][0, 0] == 2500


def test_deproject_and_the_world_render(world):
    depth, seg = world.render()
    cam = _np(world.camera())
    crop = (list(world.cfg.crop_min), list(world.cfg.crop_max))
    pts, valid = world.deproject(depth)
    want = [sh.deproject(_np(depth[e]), cam[e], crop) for e in range(world.n)]
    for e in range(world.n):
        assert np.array_equal(_np(pts[e]).view(np.uint32), want[e][0].view(np.uint32)) and np.array_equal(_np(valid[e]), want[e][1])
    # a chunk that starts at env 2 uses env 2's calibration
    pts2, valid2 = world.deproject(depth[2:], env_first=2)
    assert np.array_equal(_np(pts2), _np(pts[2:])) and np.array_equal(_np(valid2), _np(valid[2:]))
    # the whole chain, in one piece and in chunks of 3 (3 + 1 envs): the same, and equal to the restatement
    par = lib.segment_params(num_points=64, draw_index=9)
    whole = world.clustered_point_cloud(par, labels=True)
    parts = world.clustered_point_cloud(par, chunk=3, labels=True)
    ref = sh.segment_batch(np.stack([x[0] for x in want]), np.stack([x[1] for x in want]), par, sc.world_seed(world.cfg), OFFSET)
    same({k: _np(v) for k, v in whole.items()}, ref, 'whole')
    same({k: _np(v) for k, v in parts.items()}, ref, 'chunks')
    assert 'labels' not in world.clustered_point_cloud(par, chunk=3)
    assert (ref['info'][:, abi.RV_SEG_INFO_CLUSTERS] >= 1).all()


BAD_PARAMS = [dict(num_hypotheses=1025), dict(num_hypotheses=-1), dict(num_clusters=0), dict(num_clusters=17), dict(num_points=0),
              dict(num_points=65537), dict(eps=0.0), dict(eps=-1.0), dict(eps=float('inf')), dict(eps=float('nan')),
              dict(plane_thresh=0.0), dict(plane_thresh=float('nan')), dict(plane_thresh=float('inf')), dict(min_samples=0),
              dict(draw_index=1 << 32), dict(draw_index=-1)]


def test_refusals(world):
    import torch
    w = world
    pts = torch.zeros((2, 16, 3), dtype=torch.float32, device=w.device)
    outs = dict(labels=torch.zeros((2, 16), dtype=torch.int32, device=w.device), clouds=torch.zeros((2, 4, 8, 3), device=w.device),
                slot_labels=torch.zeros((2, 4), dtype=torch.int32, device=w.device), slot_counts=torch.zeros((2, 4), dtype=torch.int32, device=w.device),
                plane=torch.zeros((2, 4), device=w.device), info=torch.zeros((2, 8), dtype=torch.int32, device=w.device))
    order = ('labels', 'clouds', 'slot_labels', 'slot_counts', 'plane', 'info')

    def call(par=None, first=0, count=2, m=16, points=pts.data_ptr(), null_params=False, **ptrs):
        p = lib.segment_params(**dict(dict(num_points=8), **(par or {})))
        a = [C.c_void_p(ptrs.get(k, outs[k].data_ptr())) for k in order]
        return w.lib.rv_segment_cloud(w.h, None if null_params else C.byref(p), first, count, C.c_void_p(points), None, m, *a)

    assert call() == abi.RV_OK
    for par in BAD_PARAMS:
        assert call(par) == abi.RV_ERR_VALUE, par
        assert b'rv_segment_cloud' in w.lib.rv_last_error()
    for kw in (dict(m=0), dict(m=(1 << 24) + 1), dict(first=-1), dict(first=3, count=2), dict(count=0), dict(null_params=True),
               dict(points=0), dict(points=pts.data_ptr() + 2)):
        assert call(**kw) == abi.RV_ERR_VALUE, kw
    for k in order:
        assert call(**{k: 0}) == abi.RV_ERR_VALUE, k
        assert call(**{k: outs[k].data_ptr() + 1}) == abi.RV_ERR_VALUE, k
    with pytest.raises(ValueError):
        w.segment_cloud(pts, None, lib.segment_params(min_samples=0))
    depth = torch.zeros((2, int(w.cfg.cam_height), int(w.cfg.cam_width)), device=w.device)
    p3 = torch.zeros((2, depth.shape[1] * depth.shape[2], 3), device=w.device)
    v = torch.zeros((2, depth.shape[1] * depth.shape[2]), dtype=torch.uint8, device=w.device)
    dp = w.lib.rv_deproject
    assert dp(w.h, 0, 2, C.c_void_p(depth.data_ptr()), C.c_void_p(p3.data_ptr()), C.c_void_p(v.data_ptr())) == abi.RV_OK
    for args in ((3, 2, depth.data_ptr(), p3.data_ptr(), v.data_ptr()), (0, 0, depth.data_ptr(), p3.data_ptr(), v.data_ptr()),
                 (0, 2, 0, p3.data_ptr(), v.data_ptr()), (0, 2, depth.data_ptr(), 0, v.data_ptr()), (0, 2, depth.data_ptr(), p3.data_ptr(), 0),
                 (0, 2, depth.data_ptr() + 2, p3.data_ptr(), v.data_ptr())):
        assert dp(w.h, args[0], args[1], C.c_void_p(args[2]), C.c_void_p(args[3]), C.c_void_p(args[4])) == abi.RV_ERR_VALUE, args
    w.synchronize()


class _Env(object):
    def __init__(self, world):
        self.world = world


def test_observation_classes(world):
    from robovat_amd import observations as obs
    env = _Env(world)
    depth, _ = world.render(segmask=False)
    seg = obs.SegmentedPointCloudObs(num_points=48, num_bodies=3, env_index=2, segmentation='cluster', draw_index=4, min_samples=30)
    seg.initialize(env)
    par = lib.segment_params(num_points=48, num_clusters=3, draw_index=4, min_samples=30)
    pts, valid = world.deproject(depth[2:3], env_first=2)
    by_hand = world.segment_cloud(pts, valid, par, env_first=2)
    got = seg.get_observation()
    assert got.shape == seg.get_gym_space().shape == (3, 48, 3) and np.array_equal(got, _np(by_hand['clouds'][0]))
    pc = obs.PointCloudObs(num_points=40, env_index=1, draw_index=2)
    pc.initialize(env)
    par = lib.segment_params(num_points=40, num_clusters=1, draw_index=2, eps=1e15, min_samples=1)
    pts, valid = world.deproject(depth[1:2], env_first=1)
    by_hand = world.segment_cloud(pts, valid, par, env_first=1)
    got = pc.get_observation()
    assert got.shape == pc.get_gym_space().shape == (40, 3) and np.array_equal(got, _np(by_hand['clouds'][0, 0]))
    info = _np(by_hand['info'][0])
    assert _np(by_hand['slot_counts'])[0, 0] == info[abi.RV_SEG_INFO_KEPT] > 0 and info[abi.RV_SEG_INFO_CLUSTERS] == 1
    # the default is what it was: the segmask-grouped cloud of rv_observe
    plain = obs.SegmentedPointCloudObs(env_index=3)
    plain.initialize(env)
    assert np.array_equal(plain.get_observation(), _np(world.observe(point_cloud=True)['point_cloud'][3]))
    with pytest.raises(ValueError):
        obs.SegmentedPointCloudObs(segmentation='nope')


def test_env_methods():
    from robovat_amd.envs.push.push_env import VecPushEnv, PushEnv
    env = VecPushEnv(3, seed=3)
    env.reset()
    out = env.clustered_point_cloud(num_points=32, draw_index=1, chunk=2, min_samples=40)
    par = lib.segment_params(num_points=32, draw_index=1, min_samples=40)
    want = env.world.clustered_point_cloud(par)
    assert set(out) == {'clouds', 'slot_labels', 'slot_counts', 'plane', 'info'} and tuple(out['clouds'].shape) == (3, abi.RV_MAXB, 32, 3)
    for k in out:
        assert np.array_equal(_np(out[k]), _np(want[k])), k
    env.close()
    one = PushEnv(seed=3)
    one.reset()
    got = one.clustered_point_cloud(num_points=16)
    assert tuple(got['clouds'].shape) == (abi.RV_MAXB, 16, 3) and tuple(got['info'].shape) == (8,)
    one.close()


def test_clusters_of_the_device_render_are_the_bodies():
    """the purity statement of tests/test_segment_host.py on the device's own render, same seed: in every env that
    satisfies the precondition the kept clusters are pure and every body owns a slot; at least 3 of the 8 qualify"""
    cfg, scene = sc.push_crop_cfg(sc.E2E_ENVS)
    w = lib.World(cfg, scene, device=0)
    w.reset()
    depth, seg = w.render()
    pts, valid = w.deproject(depth)
    out = {k: _np(v) for k, v in w.clustered_point_cloud(lib.segment_params(**sc.params()), chunk=3, depth=depth, labels=True).items()}
    n_bodies = (_np(w.body_params())[:, :, 0] > 0).sum(axis=1)
    pts, valid, seg = _np(pts), _np(valid), _np(seg)
    w.close()
    qualifying = 0
    for e in range(sc.E2E_ENVS):
        if not sc.precondition(pts[e], valid[e], seg[e], int(n_bodies[e])):
            continue
        qualifying += 1
        ok, why = sc.purity({k: v[e] for k, v in out.items()}, seg[e], int(n_bodies[e]))
        assert ok, 'env %d: %s' % (e, why)
    assert qualifying >= 3, qualifying
