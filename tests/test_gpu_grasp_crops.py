"""rv_grasp_crops on the MI355X: k_grasp_crops compared bit for bit with tests/grasp_crop_host.py (its
float32 NumPy restatement) on images whose every value is unique -- tie, generic, outside and non-finite rows side by side
in one call, both store paths, wave counts around one wave per image --, the refusals, and the env level:
VecGrasp4DofEnv.grasp_images / collect_grasp_samples, Grasp4DofEnv's forms and the data set on disk."""
import ctypes as C

import numpy as np
import pytest

import grasp_crop_host as gch
from robovat_amd import abi, configs, lib, scenes
from robovat_amd.io import grasp_dataset, hdf5_utils

pytestmark = pytest.mark.gpu
F = np.float32
N = 3
POISON = -7.0
IMAGES = [(24, 32), (25, 31)]
CROPS = [
    (8, 8, 1),        # one wave per image exactly
    (7, 9, 2),        # 63 pixels: one short of a wave
    (5, 13, 1),       # 65 pixels: one over
    (16, 16, 3),      # a window larger than the image; 256 pixels: the four-pixels-per-lane kernel, one wave
    (20, 20, 1),      # 400 pixels: the four-pixels-per-lane kernel, a second wave that is partly idle
    (18, 18, 2),      # 324 pixels: at least 256 but rows of 18 -- a lane's four pixels span rows of the crop
]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope='module')
def world():
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=N,
                                 shape_names=names, seed=3)
    w = lib.World(cfg, scene, device=0)
    yield w
    w.close()


def _rows(H, W, K):
    """[N, K, 5]: tie, outside / non-finite, p1 == p2 and generic rows interleaved, in another order for every env, so that
    an ordinary row always has an all-zero neighbour and a stray write shows"""
    edge, _ = gch.edge_rows(H, W)
    pool = np.concatenate([gch.tie_rows(H, W), edge, gch.generic_rows(64, H, W, seed=H + K)])
    out = np.zeros((N, K, 5), F)
    for n in range(N):
        rng = np.random.RandomState(10 * K + n)
        if K == 1:
            out[n, 0] = pool[[0, len(gch.tie_rows(H, W)), -1][n]]      # a tie row, a NaN row, a generic row
        else:
            special = min(K // 2, len(pool) - 64)
            pick = np.concatenate([rng.permutation(len(pool) - 64)[:special], len(pool) - 64 + rng.permutation(64)[:K - special]])
            out[n] = pool[rng.permutation(pick)]
    return out


@pytest.mark.parametrize('K', [1, 5, 64])
@pytest.mark.parametrize('h,w,step', CROPS)
@pytest.mark.parametrize('H,W', IMAGES)
def test_kernel_equals_the_host_restatement(world, H, W, h, w, step, K):
    t = world.torch
    depth = gch.ramp(N, H, W)
    rows = _rows(H, W, K)
    want, want_gd = gch.crops(depth, rows, h, w, step)
    assert want.any() and (K == 1 or any(not want[n, k].any() for n in range(N) for k in range(K)))
    p = lib.grasp_crop_params(h, w, step)
    images, gd = world.grasp_crops(depth, rows, p)
    assert tuple(images.shape) == (N, K, h, w) and tuple(gd.shape) == (N, K)
    assert _same(images.cpu().numpy(), want) and _same(gd.cpu().numpy(), want_gd)
    # without the grasp depths
    images2, none = world.grasp_crops(depth, rows, p, grasp_depths=False)
    assert none is None and _same(images2.cpu().numpy(), want)
    # into a caller's tensor: 16-byte aligned, and 4-byte aligned only (one pixel per lane whatever the size); the
    # floats before and after it stay as they were
    for lead in (4, 1):
        buf = t.full((lead + want.size + 4,), POISON, dtype=t.float32, device=world.device)
        out = buf[lead:lead + want.size].view(N, K, h, w)
        assert (out.data_ptr() % 16 == 0) == (lead == 4)
        got, _ = world.grasp_crops(depth, rows, p, out=out)
        assert got is out and _same(out.cpu().numpy(), want)
        assert bool((buf[:lead] == POISON).all()) and bool((buf[lead + want.size:] == POISON).all())
    if K == 1:      # [N, 5] is K = 1
        one, gd1 = world.grasp_crops(depth, rows[:, 0], p)
        assert tuple(one.shape) == (N, 1, h, w) and _same(one.cpu().numpy(), want) and _same(gd1.cpu().numpy(), want_gd)


def test_refusals_leave_the_outputs_untouched(world):
    t = world.torch
    H, W, K = 24, 32, 2
    depth = t.as_tensor(gch.ramp(N, H, W), device=world.device)
    rows = t.as_tensor(_rows(H, W, K), device=world.device)
    images = t.full((N, abi.RV_AP_MAX_SAMPLES + 1, 8, 8), POISON, dtype=t.float32, device=world.device)
    gd = t.full((N, abi.RV_AP_MAX_SAMPLES + 1), POISON, dtype=t.float32, device=world.device)
    good = dict(height=H, width=W, crop_height=8, crop_width=8, step=1)
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def refused(params, d=depth, g=rows, k=K, out=images, dep=gd, what='rv_grasp_crops'):
        rc = world.lib.rv_grasp_crops(world.h, None if params is None else C.byref(params), ptr(d), ptr(g), k, ptr(out), ptr(dep))
        assert rc == abi.RV_ERR_VALUE and what.encode() in world.lib.rv_last_error(), (what, rc)
        world.synchronize()
        assert bool((images == POISON).all()) and bool((gd == POISON).all()), what

    ok = abi.rv_grasp_crop_params(**good)
    refused(None)
    refused(ok, d=None); refused(ok, g=None); refused(ok, out=None)
    for field, values in (('height', (0, -1)), ('width', (0, -5)),
                          ('crop_height', (0, -1, abi.RV_GC_MAX_SIDE + 1)), ('crop_width', (0, -1, abi.RV_GC_MAX_SIDE + 1)),
                          ('step', (0, -1, abi.RV_GC_MAX_STEP + 1))):
        for v in values:
            refused(abi.rv_grasp_crop_params(**dict(good, **{field: v})), what=field if field in ('height', 'step') else 'rv_grasp_crops')
    for k in (0, -1, abi.RV_AP_MAX_SAMPLES + 1):
        refused(ok, k=k, what='k outside')
    # the binding raises ValueError for them, and checks shapes, dtype and device itself
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows, lib.grasp_crop_params(0, 8, 1))
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows, lib.grasp_crop_params(8, 8, 17))
    with pytest.raises(ValueError):
        world.grasp_crops(depth, t.zeros((N, abi.RV_AP_MAX_SAMPLES + 1, 5), device=world.device), lib.grasp_crop_params(8, 8, 1))
    with pytest.raises(ValueError):
        world.grasp_crops(depth[:2], rows[:2], ok)
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows[:, :, :4], ok)
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows, ok, out=t.zeros((N, K, 8, 9), dtype=t.float32, device=world.device))
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows, ok, out=t.zeros((N, K, 8, 8), dtype=t.float64, device=world.device))
    with pytest.raises(ValueError):
        world.grasp_crops(depth, rows, ok, out=t.zeros((N, K, 8, 8), dtype=t.float32))
    # the limits themselves run
    big, _ = world.grasp_crops(depth, rows[:, :1], lib.grasp_crop_params(abi.RV_GC_MAX_SIDE, abi.RV_GC_MAX_SIDE, abi.RV_GC_MAX_STEP))
    want, _ = gch.crops(depth.cpu().numpy(), rows[:, :1].cpu().numpy(), abi.RV_GC_MAX_SIDE, abi.RV_GC_MAX_SIDE, abi.RV_GC_MAX_STEP)
    assert _same(big.cpu().numpy(), want)


def test_env_level_samples_equal_the_separate_calls_and_survive_the_disk(tmp_path):
    from robovat_amd import envs
    n, K, seed = 4, 4, 5
    crop = dict(crop_height=16, crop_width=16, step=2)
    env = envs.VecGrasp4DofEnv(n, seed=seed)
    one = envs.Grasp4DofEnv(seed=seed)
    try:
        env.reset()
        with pytest.raises(ValueError):
            env.grasp_images()      # no sampling call before it
        before = env.world.save_state().blocks.cpu().numpy()
        s = env.collect_grasp_samples(K, **crop)
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        assert sorted(s) == sorted(['images', 'grasp_depths', 'image_grasps', 'actions4', 'rewards', 'dones', 'count', 'status', 'valid'])
        assert tuple(s['images'].shape) == (n, K, 16, 16) and tuple(s['valid'].shape) == (n, K)
        # the loop of separate calls
        d, _ = env.world.render()
        env.sample_antipodal_candidates(K, depth=d)
        g, a4 = env.antipodal_image_grasps, env.antipodal_actions4
        images, gd = env.world.grasp_crops(d, g, lib.grasp_crop_params(**crop))
        r, dn = env.try_grasps(a4)
        cnt, st = env.antipodal_count.cpu().numpy(), env.antipodal_status.cpu().numpy()
        for key, v in (('images', images), ('grasp_depths', gd), ('image_grasps', g), ('actions4', a4), ('rewards', r)):
            assert _same(s[key].cpu().numpy(), v.cpu().numpy()), key
        assert np.array_equal(s['dones'].cpu().numpy(), dn.cpu().numpy())
        assert np.array_equal(s['count'].cpu().numpy(), cnt) and np.array_equal(s['status'].cpu().numpy(), st)
        valid = s['valid'].cpu().numpy()
        assert valid.dtype == np.bool_ and np.array_equal(valid, (st == 1)[:, None] & (np.arange(K)[None] < cnt[:, None]))
        assert valid.any()
        assert _same(s['grasp_depths'].cpu().numpy(), g.cpu().numpy()[:, :, 4])
        # the kernel's images are the restatement's on a real render
        want, _ = gch.crops(d.cpu().numpy(), g.cpu().numpy(), 16, 16, 2)
        assert _same(images.cpu().numpy(), want) and want.any()
        # grasp_images(): the last sampling call's grasps on a fresh render; explicit arguments; the defaults
        gi, gdi = env.grasp_images(**crop)
        assert _same(gi.cpu().numpy(), images.cpu().numpy()) and _same(gdi.cpu().numpy(), gd.cpu().numpy())
        gi, _ = env.grasp_images(g[:, 0], d, **crop)
        assert _same(gi.cpu().numpy(), images.cpu().numpy()[:, :1])
        assert tuple(env.grasp_images()[0].shape) == (n, K, 32, 32)
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        # Grasp4DofEnv (env 0 of the same seed): the vec env's row 0
        one.reset()
        with pytest.raises(ValueError):
            one.grasp_images()
        s1 = one.collect_grasp_samples(K, **crop)
        for key in s:
            assert np.array_equal(s1[key], s[key][0].cpu().numpy()), key
        i1, d1 = one.grasp_images(**crop)
        assert _same(i1, images[0].cpu().numpy()) and _same(d1, gd[0].cpu().numpy())
        i1, d1 = one.grasp_images(g[0, 1].cpu().numpy(), d[0].cpu().numpy(), **crop)
        assert _same(i1, images[0, 1:2].cpu().numpy())
        # the disk
        name = str(tmp_path / 'grasps')
        with hdf5_utils.open_store(name, 'a') as store:
            grasp_dataset.append_grasp_samples(store, s)
            grasp_dataset.append_grasp_samples(store, s1, only_valid=False)
        with hdf5_utils.open_store(name, 'r') as store:
            got = grasp_dataset.read_grasp_samples(store)
        m = int(valid.sum())
        for key in grasp_dataset.PER_SAMPLE:
            full = s[key].cpu().numpy()
            want = np.concatenate([full[valid], full[0]])
            assert got[key].dtype == want.dtype and np.array_equal(got[key], want), key
        assert len(got['env']) == m + K and np.array_equal(got['env'][:m], np.nonzero(valid)[0])
    finally:
        env.close()
        one.close()
