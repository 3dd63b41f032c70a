"""rv_ward_groups on the device: bit for bit equal to the restatement (tests/ward_host.py) in groups,
clouds, slot_counts and info, with guard words around every output and the workspace, on the clouds scikit-learn labelled,
the tie lattice, the word and wave boundaries, few points, the overflow cloud and labels as rv_segment_cloud leaves them;
chunks; every refusal; the env method and the observation class against the calls made by hand; the defaults unchanged."""
import ctypes as C

import numpy as np
import pytest

import segment_cases as sc
import ward_cases as wc
import ward_host as wh
from robovat_amd import abi, lib

pytestmark = pytest.mark.gpu
GUARD = 64
GOLDEN, _ = wc.golden()
CLOUDS = GOLDEN + [dict(name='tie_lattice', points=wc.tie_lattice(), k=6, C=3, labels=None)]
OFFSET = 5
FILL_I, FILL_F, FILL_W = 0x5A5A5A5, -77.0, 0x5A5A5A5A5A5A5A5


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


def run(w, points, labels, p, env_first=0):
    """rv_ward_groups with guard words on both sides of every output and of the workspace -> dict of NumPy arrays"""
    import torch
    pts = torch.as_tensor(np.ascontiguousarray(points, np.float32), device=w.device)
    lab = torch.as_tensor(np.ascontiguousarray(labels, np.int32), device=w.device)
    n, m = pts.shape[0], pts.shape[1]
    par = lib.ward_params(**p)
    c, q = int(par.num_groups), int(par.num_points)
    specs = dict(groups=((n, m), torch.int32, FILL_I), clouds=((n, c, q, 3), torch.float32, FILL_F),
                 slot_counts=((n, c), torch.int32, FILL_I), info=((n, 8), torch.int32, FILL_I))
    bufs = {k: _guarded(w, *s) for k, s in specs.items()}
    need = int(w.lib.rv_ward_workspace_bytes(n))
    assert need % 8 == 0
    ws, ws_view = _guarded(w, (need // 8,), torch.int64, FILL_W)
    ptr = {k: C.c_void_p(b[1].data_ptr()) for k, b in bufs.items()}
    lib.check(w.lib.rv_ward_groups(w.h, C.byref(par), int(env_first), n, C.c_void_p(pts.data_ptr()), C.c_void_p(lab.data_ptr()), m,
                                   C.c_void_p(ws_view.data_ptr()), need, ptr['groups'], ptr['clouds'], ptr['slot_counts'], ptr['info']))
    w.synchronize()
    out = {}
    for k, (buf, view) in bufs.items():
        fill = specs[k][2]
        g = _np(buf)
        assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), 'guard words of %s' % k
        out[k] = _np(view).copy()
    assert bool((ws[:GUARD] == FILL_W).all()) and bool((ws[-GUARD:] == FILL_W).all()), 'guard words of the workspace'
    return out


def same(got, want, who=''):
    for k in ('groups', 'slot_counts', 'info'):
        assert np.array_equal(got[k], want[k]), (who, k, got[k], want[k])
    assert np.array_equal(got['clouds'].view(np.uint32), np.ascontiguousarray(want['clouds'], np.float32).view(np.uint32)), (who, 'clouds')
    assert not (got['info'][:, abi.RV_WARD_INFO_FLAGS] & abi.RV_WARD_FLAG_BOUND).any()


def pad(clouds, labels=None):
    """clouds of different sizes as one [n, M, 3] batch; the padding is NaN with label RV_SEG_INVALID"""
    m = max(max(len(c) for c in clouds), 1)
    pts = np.full((len(clouds), m, 3), np.nan, np.float32)
    lab = np.full((len(clouds), m), abi.RV_SEG_INVALID, np.int32)
    for e, c in enumerate(clouds):
        pts[e, :len(c)] = c
        lab[e, :len(c)] = 0 if labels is None else labels[e]
    return pts, lab


def check(world, clouds, p, env_first=0, labels=None, who=''):
    pts, lab = pad(clouds, labels)
    got = run(world, pts, lab, p, env_first=env_first)
    same(got, wh.ward_groups_batch(pts, lab, p, sc.world_seed(world.cfg), OFFSET + env_first), who)
    return got


@pytest.mark.parametrize('k', range(len(CLOUDS)), ids=[c['name'] for c in CLOUDS])
def test_golden_clouds(world, k):
    """three different clouds in one call (envs 1 .. 3 of the world); env 0 of the call is case k with its own k and C,
    so its groups are scikit-learn's partition too"""
    cases = [CLOUDS[(k + j) % len(CLOUDS)] for j in range(3)]
    p = wc.params(num_neighbors=cases[0]['k'], num_groups=cases[0]['C'], num_points=33, draw_index=k)
    got = check(world, [c['points'] for c in cases], p, env_first=1, who=cases[0]['name'])
    if cases[0]['labels'] is not None:
        assert wh.same_partition(got['groups'][0][:len(cases[0]['points'])], cases[0]['labels'])
    assert (got['info'][:, abi.RV_WARD_INFO_GROUPS] == cases[0]['C']).all()


def test_word_and_wave_boundaries(world):
    sizes = (63, 64, 65, 129)
    clouds = [wc.sized_cloud(n, n) for n in sizes]
    got = check(world, clouds, wc.params(num_neighbors=10, num_groups=3, num_points=64), who='k 10')
    assert got['info'][:, abi.RV_WARD_INFO_KEPT].tolist() == list(sizes)
    # n = k + 1 (the complete graph) at 65 and at 129; 63 and 64 are then below k + 1
    check(world, clouds[:3], wc.params(num_neighbors=64, num_groups=2, num_points=65), env_first=1, who='k 64')
    check(world, [clouds[3], clouds[2], clouds[1]], wc.params(num_neighbors=128, num_groups=5, num_points=1), who='k 128')
    # one neighbour: many components, many completion edges
    got = check(world, clouds, wc.params(num_neighbors=1, num_groups=16, num_points=9), who='k 1')
    assert (got['info'][:, abi.RV_WARD_INFO_COMPONENTS] > 3).all()


def test_few_points(world):
    clouds = [wc.sized_cloud(n, 50 + n) for n in (0, 1, 3, 4)]
    got = check(world, clouds, wc.params(num_neighbors=3, num_groups=4, num_points=6), who='few')
    assert got['info'][:, abi.RV_WARD_INFO_GROUPS].tolist() == [0, 1, 3, 4]
    assert [bool(f & abi.RV_WARD_FLAG_FEWER) for f in got['info'][:, abi.RV_WARD_INFO_FLAGS]] == [True, True, True, False]
    assert (got['clouds'][0] == 0).all() and got['slot_counts'][2].tolist() == [1, 1, 1, 0]
    check(world, [wc.sized_cloud(5, 3)], wc.params(num_neighbors=100, num_groups=4, num_points=2), env_first=3, who='C + 1')


def test_overflow_cloud(world):
    pts = wc.overflow_cloud()
    got = check(world, [pts], wc.params(num_neighbors=8, num_groups=4, num_points=300), env_first=2, who='overflow')
    info = got['info'][0]
    assert info[abi.RV_WARD_INFO_INPUT] == 2500 and info[abi.RV_WARD_INFO_KEPT] == abi.RV_WARD_MAXPTS
    assert info[abi.RV_WARD_INFO_FLAGS] == abi.RV_WARD_FLAG_OVERFLOW and (got['groups'][0] == abi.RV_SEG_SKIPPED).sum() == 2500 - abi.RV_WARD_MAXPTS


def test_labels_as_segment_cloud_leaves_them(world):
    pts, lab = wc.mixed_cloud()
    got = check(world, [pts, pts[::-1]], wc.params(num_neighbors=12, num_groups=3, num_points=16), labels=[lab, lab[::-1]], who='mixed')
    assert np.array_equal(got['groups'][0][lab < 0], lab[lab < 0])
    assert (got['groups'][0][(lab >= 0) & ~np.isfinite(pts).all(axis=1)] == abi.RV_SEG_INVALID).all()


def test_chunks_and_the_world_method(world):
    """4 envs whole and as 3 + 1 through World.ward_groups (its own workspace, grown from 1 env to 3): the same, and equal
    to the restatement; the draws follow the global env id"""
    clouds = [c['points'] for c in GOLDEN[:4]]
    pts, lab = pad(clouds)
    par = lib.ward_params(num_points=40, num_groups=3, num_neighbors=20, draw_index=9)
    last = {k: _np(v) for k, v in world.ward_groups(pts[3:], lab[3:], par, env_first=3).items()}
    first = {k: _np(v) for k, v in world.ward_groups(pts[:3], lab[:3], par).items()}
    whole = {k: _np(v) for k, v in world.ward_groups(pts, lab, par).items()}
    want = wh.ward_groups_batch(pts, lab, par, sc.world_seed(world.cfg), OFFSET)
    same(whole, want, 'whole')
    same({k: np.concatenate([first[k], last[k]]) for k in whole}, want, 'chunks')
    moved = {k: _np(v) for k, v in world.ward_groups(pts[:1], lab[:1], par, env_first=2).items()}
    assert np.array_equal(moved['groups'], whole['groups'][:1]) and not np.array_equal(moved['clouds'], whole['clouds'][:1])


BAD_PARAMS = [dict(num_neighbors=0), dict(num_neighbors=129), dict(num_groups=0), dict(num_groups=17), dict(num_points=0),
              dict(num_points=65537), dict(draw_index=1 << 32), dict(draw_index=-1)]


def test_refusals(world):
    import torch
    w = world
    pts = torch.zeros((2, 16, 3), dtype=torch.float32, device=w.device)
    lab = torch.zeros((2, 16), dtype=torch.int32, device=w.device)
    need = int(w.lib.rv_ward_workspace_bytes(2))
    ws = torch.zeros((need // 8 + 1,), dtype=torch.int64, device=w.device)
    outs = dict(groups=torch.zeros((2, 16), dtype=torch.int32, device=w.device), clouds=torch.zeros((2, 4, 8, 3), device=w.device),
                slot_counts=torch.zeros((2, 4), dtype=torch.int32, device=w.device), info=torch.zeros((2, 8), dtype=torch.int32, device=w.device))
    order = ('groups', 'clouds', 'slot_counts', 'info')

    def call(par=None, first=0, count=2, m=16, points=pts.data_ptr(), labels=lab.data_ptr(), workspace=ws.data_ptr(), nbytes=need,
             null_params=False, **ptrs):
        p = lib.ward_params(**dict(dict(num_points=8), **(par or {})))
        a = [C.c_void_p(ptrs.get(k, outs[k].data_ptr())) for k in order]
        return w.lib.rv_ward_groups(w.h, None if null_params else C.byref(p), first, count, C.c_void_p(points), C.c_void_p(labels), m,
                                    C.c_void_p(workspace), nbytes, *a)

    assert call() == abi.RV_OK
    for par in BAD_PARAMS:
        assert call(par) == abi.RV_ERR_VALUE, par
        assert b'rv_ward_groups' in w.lib.rv_last_error()
    for kw in (dict(m=0), dict(m=(1 << 24) + 1), dict(first=-1), dict(first=3, count=2), dict(count=0), dict(null_params=True),
               dict(points=0), dict(points=pts.data_ptr() + 2), dict(labels=0), dict(labels=lab.data_ptr() + 2), dict(workspace=0),
               dict(workspace=ws.data_ptr() + 4), dict(nbytes=need - 1), dict(nbytes=0)):
        assert call(**kw) == abi.RV_ERR_VALUE, kw
    for k in order:
        assert call(**{k: 0}) == abi.RV_ERR_VALUE, k
        assert call(**{k: outs[k].data_ptr() + 1}) == abi.RV_ERR_VALUE, k
    assert call(workspace=ws.data_ptr() + 8) == abi.RV_OK      # (8-byte aligned, still large enough)
    with pytest.raises(ValueError):
        w.ward_groups(pts, lab, lib.ward_params(num_neighbors=0))
    with pytest.raises(ValueError):
        w.ward_groups(pts, lab[:, :5], lib.ward_params())
    w.synchronize()


class _Env(object):
    def __init__(self, world):
        self.world = world


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(_np(a[k]), _np(b[k])), k


def test_chained_call_and_observation_class(world):
    from robovat_amd import observations as obs
    par = lib.segment_params(num_points=48, num_clusters=3, draw_index=4, min_samples=30)
    ward = lib.ward_params(num_points=48, num_groups=3, num_neighbors=20, draw_index=4)
    depth, _ = world.render(segmask=False)
    # the chain, whole and in chunks, against the three calls made by hand
    pts, valid = world.deproject(depth)
    seg = world.segment_cloud(pts, valid, par)
    by_hand = world.ward_groups(pts, seg['labels'], ward)
    for chunk in (256, 3):
        got = world.clustered_point_cloud(par, chunk=chunk, depth=depth, labels=True, ward=ward)
        assert set(got) == {'clouds', 'labels', 'slot_labels', 'slot_counts', 'plane', 'info', 'ward_info', 'groups'}
        _equal({k: got[k] for k in ('clouds', 'slot_counts', 'ward_info', 'groups')},
               dict(clouds=by_hand['clouds'], slot_counts=by_hand['slot_counts'], ward_info=by_hand['info'], groups=by_hand['groups']))
        _equal({k: got[k] for k in ('labels', 'slot_labels', 'plane', 'info')}, {k: seg[k] for k in ('labels', 'slot_labels', 'plane', 'info')})
    assert set(world.clustered_point_cloud(par, depth=depth, ward=ward)) == {'clouds', 'slot_labels', 'slot_counts', 'plane', 'info', 'ward_info'}
    info = _np(by_hand['info'])
    assert (info[:, abi.RV_WARD_INFO_GROUPS] == 3).all() and (_np(by_hand['slot_counts']) > 0).all()
    assert not (info[:, abi.RV_WARD_INFO_FLAGS] & (abi.RV_WARD_FLAG_BOUND | abi.RV_WARD_FLAG_FEWER)).any()
    assert (_np(by_hand['slot_counts']).sum(axis=1) == info[:, abi.RV_WARD_INFO_KEPT]).all()      # a partition of what DBSCAN kept
    # the observation class
    env = _Env(world)
    o = obs.SegmentedPointCloudObs(num_points=48, num_bodies=3, env_index=2, segmentation='cluster', draw_index=4, min_samples=30,
                                   grouping='ward', num_neighbors=20)
    o.initialize(env)
    got = o.get_observation()
    one = world.ward_groups(pts[2:3], seg['labels'][2:3], ward, env_first=2)
    assert got.shape == o.get_gym_space().shape == (3, 48, 3) and np.array_equal(got, _np(one['clouds'][0]))
    assert np.array_equal(got, _np(by_hand['clouds'][2]))
    with pytest.raises(ValueError):
        obs.SegmentedPointCloudObs(segmentation='cluster', grouping='nope')


def test_defaults_are_unchanged(world):
    """without the new arguments every entry point returns what it returned: the same keys, the same bits as the explicit
    grouping='largest' and as rv_segment_cloud called by hand"""
    from robovat_amd import observations as obs
    par = lib.segment_params(num_points=32, draw_index=1, min_samples=40)
    depth, _ = world.render(segmask=False)
    pts, valid = world.deproject(depth)
    seg = world.segment_cloud(pts, valid, par)
    plain = world.clustered_point_cloud(par, depth=depth)
    assert set(plain) == {'clouds', 'slot_labels', 'slot_counts', 'plane', 'info'}
    _equal(plain, {k: seg[k] for k in plain})
    _equal(world.clustered_point_cloud(par, depth=depth, ward=None), plain)
    o = obs.SegmentedPointCloudObs(num_points=32, env_index=1, segmentation='cluster', draw_index=1, min_samples=40)
    o.initialize(_Env(world))
    assert o.grouping == 'largest' and np.array_equal(o.get_observation(), _np(seg['clouds'][1]))


def test_env_methods():
    from robovat_amd.envs.push.push_env import VecPushEnv, PushEnv
    env = VecPushEnv(3, seed=3)
    env.reset()
    plain = env.clustered_point_cloud(num_points=32, draw_index=1, chunk=2, min_samples=40)
    _equal(env.clustered_point_cloud(num_points=32, draw_index=1, chunk=2, min_samples=40, grouping='largest'), plain)
    out = env.clustered_point_cloud(num_points=32, draw_index=1, chunk=2, min_samples=40, grouping='ward', num_neighbors=30, labels=True)
    want = env.world.clustered_point_cloud(lib.segment_params(num_points=32, draw_index=1, min_samples=40), labels=True,
                                           ward=lib.ward_params(num_points=32, num_neighbors=30, draw_index=1))
    assert set(out) == set(plain) | {'ward_info', 'labels', 'groups'} and tuple(out['clouds'].shape) == (3, abi.RV_MAXB, 32, 3)
    _equal(out, want)
    _equal({k: out[k] for k in ('slot_labels', 'plane', 'info')}, {k: plain[k] for k in ('slot_labels', 'plane', 'info')})
    assert (_np(out['ward_info'])[:, abi.RV_WARD_INFO_GROUPS] == abi.RV_MAXB).all() and (_np(out['slot_counts']) > 0).all()
    with pytest.raises(ValueError):
        env.clustered_point_cloud(grouping='nope')
    env.close()
    one = PushEnv(seed=3)
    one.reset()
    got = one.clustered_point_cloud(num_points=16, grouping='ward')
    assert tuple(got['clouds'].shape) == (abi.RV_MAXB, 16, 3) and tuple(got['ward_info'].shape) == (8,)
    one.close()
