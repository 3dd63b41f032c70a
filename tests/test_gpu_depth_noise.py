"""rv_depth_noise on the MI355X: the two kernels of csrc/rv_dev_depth_noise.h compared bit for bit with
tests/depth_noise_host.py (its float32 NumPy restatement) -- the recorded draws, the output, in place, the world's own
scratch grid, every tile seam of the product's 424 x 512 image --, the switches, the independence of an env's noise from
the batch, the refusals, and the observation of VecGrasp4DofEnv with OBSERVATION.DEPTH_NOISE set."""
import ctypes as C

import numpy as np
import pytest

import depth_noise_host as host
from robovat_amd import abi, configs, lib, scenes
from robovat_amd.envs.grasp.grasp_4dof_env import VecGrasp4DofEnv

pytestmark = pytest.mark.gpu
F = np.float32
N, OFFSET, SEED = 3, 5, 7 + (5 << 32)
SEED_LO, SEED_HI = SEED & 0xFFFFFFFF, SEED >> 32
SHAPES = [(8, 12, 4), (24, 32, 4), (10, 14, 2), (6, 6, 1)]
NOISE = {'GAMMA_SHAPE': 1000.0, 'PROB': 0.5, 'RESCALE_FACTOR': 4, 'SIGMA': 0.005, 'SEED': 3}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _world(n, offset=0, seed=SEED):
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n,
                                 shape_names=names, env_id_offset=offset, seed=seed)
    return lib.World(cfg, scene, device=0)


@pytest.fixture(scope='module')
def world():
    w = _world(N, OFFSET)
    yield w
    w.close()


def _depth(n, height, width, seed):
    """depths around 0.7 m with scattered zeros, a negative and a negative zero (neither takes the Gaussian term)"""
    rng = np.random.RandomState(seed)
    d = rng.uniform(0.4, 1.0, (n, height, width)).astype(F)
    d[rng.uniform(size=d.shape) < 0.15] = 0.0
    d[0, 0, 0], d[0, 0, 1] = -0.5, -0.0
    return d


def _host(depth, p, gids):
    """(out, g, applied, grid) of the restatement for the envs `gids`"""
    drawn = [host.draws(SEED_LO, SEED_HI, gid, p) for gid in gids]
    g = np.array([d[0] for d in drawn], F)
    applied = np.array([d[1] for d in drawn], np.uint8)
    grid = np.stack([d[2] for d in drawn])
    return host.apply(depth, g, applied, grid, p.rescale_factor), g, applied, grid


@pytest.mark.parametrize('height,width,R', SHAPES)
def test_draws_and_output_equal_the_host_restatement(world, height, width, R):
    t = world.torch
    depth = _depth(N, height, width, seed=height)
    for k, prob, sigma, di in ((1000.0, 0.5, 0.005, 0), (2.0, 1.0, 0.01, 77), (0.0, 0.5, 0.02, (1 << 24) - 1), (50.0, 0.7, 0.0, 3)):
        p = lib.depth_noise_params(NOISE, gamma_shape=k, prob=prob, sigma=sigma, rescale_factor=R, draw_index=di,
                                   height=height, width=width)
        want, g, applied, grid = _host(depth, p, range(OFFSET, OFFSET + N))
        out, dg, da, dgrid = world.depth_noise(depth, p, record=True)
        assert _same(dg.cpu().numpy(), g) and _same(da.cpu().numpy(), applied), (k, prob, sigma)
        assert _same(dgrid.cpu().numpy(), grid)
        assert _same(out.cpu().numpy(), want), (k, prob, sigma)
        # the world's own scratch grid (d_grid NULL) gives the same output; so does writing over the input
        assert _same(world.depth_noise(depth, p).cpu().numpy(), want)
        buf = t.as_tensor(depth, device=world.device).clone()
        assert world.depth_noise(buf, p, out=buf) is buf and _same(buf.cpu().numpy(), want)
    assert applied.tolist() == host.scalars(SEED_LO, SEED_HI, np.arange(OFFSET, OFFSET + N), host.fields(p))[1].tolist()
    # buffers that are only 4-byte aligned take the one-pixel-per-lane kernel: the same values
    src = t.zeros(depth.size + 1, dtype=t.float32, device=world.device)
    dst = t.full((depth.size + 1,), -7.0, dtype=t.float32, device=world.device)
    src[1:] = t.as_tensor(depth.reshape(-1), device=world.device)
    assert src[1:].data_ptr() % 16 != 0
    p = lib.depth_noise_params(NOISE, prob=1.0, rescale_factor=R, draw_index=9, height=height, width=width)
    lib.check(world.lib.rv_depth_noise(world.h, C.byref(p), C.c_void_p(src[1:].data_ptr()), C.c_void_p(dst[1:].data_ptr()), None, None, None))
    assert _same(dst[1:].cpu().numpy().reshape(depth.shape), _host(depth, p, range(OFFSET, OFFSET + N))[0]) and float(dst[0]) == -7.0


def test_every_tile_seam_of_the_product_image():
    """2 envs at 424 x 512, R = 4 (grid 106 x 128): 8 x 14 tiles of 64 x 32 pixels per env, the last row of tiles 8 rows
    high; bit for bit, also through the one-pixel-per-lane kernel (32 x 14 tiles of 16 x 32)."""
    w = _world(2, OFFSET)
    try:
        t = w.torch
        depth = _depth(2, 424, 512, seed=1)
        p = lib.depth_noise_params(NOISE, prob=1.0, draw_index=4, height=424, width=512)
        want, g, applied, grid = _host(depth, p, (OFFSET, OFFSET + 1))
        assert applied.tolist() == [1, 1]
        out, dg, da, dgrid = w.depth_noise(depth, p, record=True)
        assert _same(dgrid.cpu().numpy(), grid) and _same(dg.cpu().numpy(), g)
        got = out.cpu().numpy()
        bad = np.argwhere(_bits(got) != _bits(want))
        assert bad.size == 0, 'first differing pixels (env, y, x): %s' % bad[:8].tolist()
        src = t.zeros(depth.size + 1, dtype=t.float32, device=w.device)
        src[1:] = t.as_tensor(depth.reshape(-1), device=w.device)
        dst = t.zeros_like(src)
        lib.check(w.lib.rv_depth_noise(w.h, C.byref(p), C.c_void_p(src[1:].data_ptr()), C.c_void_p(dst[1:].data_ptr()), None, None, None))
        assert _same(dst[1:].cpu().numpy().reshape(depth.shape), want)
    finally:
        w.close()


def test_switches(world):
    depth = _depth(N, 24, 32, seed=2)
    base = dict(height=24, width=32, draw_index=1)
    # prob 0: the gamma product alone
    p = lib.depth_noise_params(NOISE, prob=0.0, **base)
    out, g, applied, grid = world.depth_noise(depth, p, record=True)
    assert applied.cpu().numpy().tolist() == [0] * N and not grid.any()
    assert _same(out.cpu().numpy(), (depth * g.cpu().numpy()[:, None, None]).astype(F))
    assert len(set(g.cpu().numpy().tolist())) == N and np.all(g.cpu().numpy() != 1.0)
    # gamma off and sigma 0: a bitwise copy, whatever the flag says
    p = lib.depth_noise_params(NOISE, gamma_shape=0.0, sigma=0.0, prob=1.0, **base)
    out, g, applied, grid = world.depth_noise(depth, p, record=True)
    assert _same(out.cpu().numpy(), depth) and g.cpu().numpy().tolist() == [1.0] * N
    # prob 1: every env
    p = lib.depth_noise_params(NOISE, prob=1.0, **base)
    out, g, applied, grid = world.depth_noise(depth, p, record=True)
    assert applied.cpu().numpy().tolist() == [1] * N and grid.cpu().numpy().std() > 0.003
    o = out.cpu().numpy()
    changed = o != (depth * g.cpu().numpy()[:, None, None]).astype(F)
    assert changed[depth > 0].mean() > 0.99 and not changed[depth <= 0].any()


def test_an_envs_noise_does_not_depend_on_the_batch():
    depth = _depth(4, 24, 32, seed=3)
    p = lib.depth_noise_params(NOISE, prob=1.0, draw_index=6, height=24, width=32)
    w4 = _world(4, 10)
    try:
        out4, g4, a4, grid4 = [x.cpu().numpy() for x in w4.depth_noise(depth, p, record=True)]
    finally:
        w4.close()
    for i in (0, 3):
        w1 = _world(1, 10 + i)
        try:
            out1, g1, a1, grid1 = [x.cpu().numpy() for x in w1.depth_noise(depth[i:i + 1], p, record=True)]
        finally:
            w1.close()
        assert _same(out1[0], out4[i]) and _same(g1[0], g4[i]) and _same(grid1[0], grid4[i]) and a1[0] == a4[i]
    assert not np.array_equal(grid4[0], grid4[3])


def test_refusals_launch_nothing(world):
    t = world.torch
    height, width = 8, 12
    depth = t.as_tensor(_depth(N, height, width, seed=4), device=world.device)
    out = t.full_like(depth, -3.0)
    g = t.full((N,), -3.0, dtype=t.float32, device=world.device)
    ok = dict(height=height, width=width, draw_index=0)

    def call(p, src=depth, dst=out, gamma=g, grid=None):
        ptr = lambda x: None if x is None else (C.c_void_p(x) if isinstance(x, int) else C.c_void_p(x.data_ptr()))
        return world.lib.rv_depth_noise(world.h, None if p is None else C.byref(p), ptr(src), ptr(dst), ptr(gamma), None, ptr(grid))

    good = lib.depth_noise_params(NOISE, **ok)
    bad = [
        ('null params', lambda: call(None)),
        ('null buffer', lambda: call(good, src=None)),
        ('null buffer', lambda: call(good, dst=None)),
        ('4-byte aligned', lambda: call(good, src=depth.data_ptr() + 2)),
        ('4-byte aligned', lambda: call(good, dst=out.data_ptr() + 1)),
        ('4-byte aligned', lambda: call(good, gamma=g.data_ptr() + 2)),
        ('4-byte aligned', lambda: call(good, grid=out.data_ptr() + 2)),
        ('rescale_factor outside', lambda: call(lib.depth_noise_params(NOISE, rescale_factor=0, **ok))),
        ('rescale_factor outside', lambda: call(lib.depth_noise_params(NOISE, rescale_factor=9, **ok))),
        ('rescale_factor outside', lambda: call(lib.depth_noise_params(dict(NOISE, RESCALE_FACTOR=2.5), **ok))),
        ('must divide', lambda: call(lib.depth_noise_params(NOISE, rescale_factor=3, **ok))),       # 8 % 3
        ('must divide', lambda: call(lib.depth_noise_params(NOISE, rescale_factor=8, **ok))),       # 12 % 8
        ('height or width', lambda: call(lib.depth_noise_params(NOISE, height=0, width=12))),
        ('draw_index', lambda: call(lib.depth_noise_params(NOISE, height=height, width=width, draw_index=-1))),
        ('draw_index', lambda: call(lib.depth_noise_params(NOISE, height=height, width=width, draw_index=1 << 24))),
        ('gamma_shape', lambda: call(lib.depth_noise_params(NOISE, gamma_shape=0.5, **ok))),
        ('gamma_shape', lambda: call(lib.depth_noise_params(NOISE, gamma_shape=-1.0, **ok))),
        ('gamma_shape', lambda: call(lib.depth_noise_params(NOISE, gamma_shape=np.nan, **ok))),
        ('prob', lambda: call(lib.depth_noise_params(NOISE, prob=-0.01, **ok))),
        ('prob', lambda: call(lib.depth_noise_params(NOISE, prob=1.01, **ok))),
        ('prob', lambda: call(lib.depth_noise_params(NOISE, prob=np.nan, **ok))),
        ('sigma', lambda: call(lib.depth_noise_params(NOISE, sigma=-1e-6, **ok))),
        ('sigma', lambda: call(lib.depth_noise_params(NOISE, sigma=np.nan, **ok))),
        # 3 envs x 2^30 x 2^30 pixels: more workgroups than a launch takes (no buffer is touched before the refusal)
        ('too many pixels', lambda: call(lib.depth_noise_params(NOISE, height=1 << 30, width=1 << 30, draw_index=0))),
    ]
    for text, fn in bad:
        rc = fn()
        assert rc == abi.RV_ERR_VALUE, text
        with pytest.raises(ValueError, match=text):
            lib.check(rc)
    world.synchronize()
    assert bool((out == -3.0).all()) and bool((g == -3.0).all())
    # the Python layer: shapes and the out tensor
    with pytest.raises(ValueError):
        world.depth_noise(depth[:2], good)
    with pytest.raises(ValueError):
        world.depth_noise(depth, good, out=t.zeros((N, height, width), dtype=t.float64, device=world.device))
    with pytest.raises(ValueError):
        world.depth_noise(depth, lib.depth_noise_params(NOISE, rescale_factor=5))
    # and the call it refuses nothing of
    assert call(good) == abi.RV_OK
    world.synchronize()
    assert bool((out != -3.0).all()) and bool((g != -3.0).all())


def test_env_observation_carries_the_noise():
    """VecGrasp4DofEnv with DEPTH_NOISE against a twin without it: same seed and actions, 2 envs, 2 steps.  The noise
    changes nothing but the depth: rewards, dones and the saved env blocks are identical; the noisy depth is
    apply(the twin's render, draws(...)) with draw_index 0 for reset() and k for step k; with None the depth is the
    render."""
    seed, offset = 11, 2
    noisy_cfg = configs.grasp_env_config()
    noisy_cfg.OBSERVATION.DEPTH_NOISE = dict(NOISE, PROB=1.0)
    clean = VecGrasp4DofEnv(2, configs.grasp_env_config(), seed=seed, env_id_offset=offset)
    noisy = VecGrasp4DofEnv(2, noisy_cfg, seed=seed, env_id_offset=offset)
    try:
        assert clean.config.OBSERVATION.DEPTH_NOISE is None
        c = clean.rv_config
        height, width = int(c.cam_height), int(c.cam_width)

        def check(obs_clean, obs_noisy, index):
            render = clean.world.render()[0].cpu().numpy()
            assert _same(obs_clean['depth'].cpu().numpy(), render)
            p = lib.depth_noise_params(noisy_cfg.OBSERVATION.DEPTH_NOISE, draw_index=index, height=height, width=width)
            drawn = [host.draws(int(c.seed_lo), int(c.seed_hi), offset + n, p) for n in range(2)]
            want = host.apply(render, [d[0] for d in drawn], [d[1] for d in drawn], np.stack([d[2] for d in drawn]), p.rescale_factor)
            got = obs_noisy['depth'].cpu().numpy()
            assert _same(got, want) and not np.array_equal(got, render)
            for key in ('intrinsics', 'translation', 'rotation'):
                assert np.array_equal(obs_clean[key], obs_noisy[key])
            return got

        first = check(clean.reset(), noisy.reset(), 0)
        assert _same(noisy.get_observation()['depth'].cpu().numpy(), first)      # (asked again: the same noise)
        seen = [first]
        for k in (1, 2):
            actions = clean.sample_random_actions()
            oc, rc, dc, _ = clean.step(actions)
            on, rn, dn, _ = noisy.step(actions)
            assert _same(rc.cpu().numpy(), rn.cpu().numpy()) and np.array_equal(dc.cpu().numpy(), dn.cpu().numpy())
            seen.append(check(oc, on, k))
            assert np.array_equal(clean.save_state().blocks.cpu().numpy(), noisy.save_state().blocks.cpu().numpy())
        # the sampler renders a clean image of its own; handed the observation's depth it sees the noise
        a_clean = clean.sample_antipodal_actions().cpu().numpy()
        assert _same(noisy.sample_antipodal_actions().cpu().numpy(), a_clean)
    finally:
        clean.close()
        noisy.close()
