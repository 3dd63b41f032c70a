"""rv_grasp_quality on the MI355X: k_grasp_quality compared bit for bit with tests/grasp_quality_host.py
(its float32 NumPy restatement) for the default, the tiny and an 8 x 12 model at sample counts around the 8-sample batch
of a workgroup, with exact zeros in the images, pre-activations that cancel to +0 and -0, NaN samples, guard words around
the caller's tensor, the refusals and the limits of the ranges; then the env level (grasp_qualities) and
GraspQualityPolicy."""
import ctypes as C

import numpy as np
import pytest

import grasp_quality_host as gqh
from robovat_amd import abi, configs, lib, scenes
from robovat_amd.perception import grasp_quality as gq
from robovat_amd.perception.grasp_quality import GraspQualityModel

pytestmark = pytest.mark.gpu
F = np.float32
POISON = -7.0
BATCH = 8      # RV_GQ_BATCH of csrc/rv_dev_grasp_quality.h: samples per workgroup
NORM = dict(im_mean=0.45, im_inv_std=3.7, z_mean=0.55, z_inv_std=19.0)
MODELS = {
    'default': dict(gq.DEFAULT_SIZES),
    'tiny': dict(gq.TINY_SIZES),
    '8x12': dict(height=8, width=12, c1=8, c2=12, f1=20, f2=12, p=4),
}
# (N, K): N K = 1, 5, one more than a workgroup's batch, and 3 x 64 (24 workgroups, K at its limit)
SHAPES = [(1, 1), (1, 5), (1, BATCH + 1), (3, 64)]
TOTAL = 3 * 64


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope='module')
def worlds():
    """a world of 1 env and one of 3: rv_grasp_quality takes N, the device and the stream from it and nothing else"""
    scene, names = scenes.make_scene()
    out = {}
    for n in (1, 3):
        cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n,
                                     shape_names=names, seed=3)
        out[n] = lib.World(cfg, scene, device=0)
    yield out
    for w in out.values():
        w.close()


_REFERENCE = {}


def _reference(name):
    """(model, images [192, h, w], depths [192], restatement logits [192]) of a model, computed once; samples are
    independent, so every shape is a prefix of it.  A few images are all zero (a crop outside the image)."""
    if name not in _REFERENCE:
        m = GraspQualityModel.random_init(11, norm=NORM, **MODELS[name])
        x, z = gqh.sample_inputs(5, TOTAL, m.sizes['height'], m.sizes['width'])
        x[3] = 0
        x[BATCH] = 0
        _REFERENCE[name] = (m, x, z, gqh.forward(m.params, m.norm, x, z))
    return _REFERENCE[name]


@pytest.mark.parametrize('n,k', SHAPES)
@pytest.mark.parametrize('name', sorted(MODELS))
def test_kernel_equals_the_host_restatement(worlds, name, n, k):
    world = worlds[n]
    t = world.torch
    m, x, z, want = _reference(name)
    h, w = m.sizes['height'], m.sizes['width']
    rows = n * k
    xs, zs, want = x[:rows].reshape(n, k, h, w), z[:rows].reshape(n, k), want[:rows].reshape(n, k)
    assert np.isfinite(want).all() and (rows == 1 or len(set(want.ravel().tolist())) > 1)
    got = world.grasp_quality(xs, zs, m)
    assert tuple(got.shape) == (n, k) and got.dtype == t.float32
    differ = int((_bits(got.cpu().numpy()) != _bits(want)).sum())
    print('%s N = %d K = %d: %d of %d logits differ from the restatement' % (name, n, k, differ, rows))
    assert differ == 0
    # into a caller's tensor, 16-byte aligned and 4-byte aligned only; the floats before and after it stay as they were
    for lead in (4, 1):
        buf = t.full((lead + rows + 4,), POISON, dtype=t.float32, device=world.device)
        out = buf[lead:lead + rows].view(n, k)
        assert (out.data_ptr() % 16 == 0) == (lead == 4)
        assert world.grasp_quality(xs, zs, m, out=out) is out and _same(out.cpu().numpy(), want)
        assert bool((buf[:lead] == POISON).all()) and bool((buf[lead + rows:] == POISON).all())
    if k == 1:      # [N, h, w] and [N] are K = 1
        assert _same(world.grasp_quality(xs[:, 0], zs[:, 0], m).cpu().numpy(), want)


@pytest.mark.parametrize('name', ['tiny', '8x12'])
def test_pre_activations_that_cancel_to_zero_of_either_sign(worlds, name):
    world = worlds[1]
    sizes = MODELS[name]
    h, w = sizes['height'], sizes['width']
    k = BATCH + 3
    x, z = gqh.sample_inputs(9, k, h, w)
    x[:, 1::3, 2::3] = F(0.625)
    norm = dict(im_mean=0.0, im_inv_std=1.0, z_mean=0.0, z_inv_std=1.0)
    # (a) a seeded model whose conv1 channel 0 is "pixel - 0.625" (exactly +0 on those pixels), whose conv1 channel 1 and
    # conv2 channel 0 have -0 weights and a -0 bias (pre-activation -0 everywhere: relu makes +0 of it)
    m = GraspQualityModel.random_init(2, norm=norm, **sizes)
    q = m.params
    q['conv1.weight'][0] = 0; q['conv1.weight'][0, 0, 2, 2] = 1; q['conv1.bias'][0] = F(-0.625)
    q['conv1.weight'][1] = F(-0.0); q['conv1.bias'][1] = F(-0.0)
    q['conv2.weight'][0] = F(-0.0); q['conv2.bias'][0] = F(-0.0)
    # (b) every weight and bias -0: each layer's pre-activation is -0, each relu must return +0, and the logit
    # fma(+0, -0, -0) = -0 -- had a relu (or a padded MFMA operand) let a -0 through, it would be +0
    zero = GraspQualityModel({key: np.full(s, -0.0, F) for key, s in gq.param_shapes(**sizes).items()}, norm, **sizes)
    for model, what in ((m, 'cancel'), (zero, 'minus zero')):
        want = gqh.forward(model.params, model.norm, x, z)
        got = world.grasp_quality(x[None], z[None], model).cpu().numpy()[0]
        assert np.array_equal(_bits(got), _bits(want)), what
    assert np.array_equal(_bits(want), np.full(k, 0x80000000, np.uint32))


def test_a_nan_sample_changes_no_other_logit(worlds):
    world = worlds[1]
    m, x, z, want = _reference('8x12')
    k = 2 * BATCH + 2
    x, z = x[:k].copy(), z[:k].copy()
    x[5, 2, 3] = np.nan
    x[5, 7, 11] = np.inf
    x[BATCH + 1] = np.nan
    z[7] = np.nan
    changed = [5, 7, BATCH + 1]
    host = gqh.forward(m.params, m.norm, x, z)
    got = world.grasp_quality(x[None], z[None], m).cpu().numpy()[0]
    assert np.array_equal(_bits(got), _bits(host))
    keep = np.setdiff1d(np.arange(k), changed)
    assert np.array_equal(_bits(got[keep]), _bits(want[:k][keep]))
    assert not np.array_equal(_bits(got[changed]), _bits(want[:k][changed]))


def test_refusals_leave_the_output_untouched_and_the_limits_run(worlds):
    world = worlds[1]
    t = world.torch
    m, x, z, want = _reference('tiny')
    K = 4
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device=world.device)
    images, depths = dev(np.concatenate([x[:K].ravel(), np.zeros(4, F)])), dev(np.concatenate([z[:K], np.zeros(4, F)]))
    weights = dev(np.concatenate([m.blob(), np.zeros(4, F)]))
    logits = t.full((abi.RV_AP_MAX_SAMPLES + 8,), POISON, dtype=t.float32, device=world.device)
    fn = world.lib.rv_grasp_quality
    ptr = lambda v, off=0: None if v is None else C.c_void_p(v.data_ptr() + off)

    def refused(desc, wts=weights, img=images, dep=depths, k=K, out=logits, off=(0, 0, 0, 0), what='rv_grasp_quality'):
        rc = fn(world.h, None if desc is None else C.byref(desc), ptr(wts, off[0]), ptr(img, off[1]), ptr(dep, off[2]), k, ptr(out, off[3]))
        assert rc == abi.RV_ERR_VALUE and what.encode() in world.lib.rv_last_error(), (what, rc)
        world.synchronize()
        assert bool((logits == POISON).all()), what

    ok = m.descriptor()
    refused(None, what='null model')
    refused(ok, wts=None); refused(ok, img=None); refused(ok, dep=None); refused(ok, out=None)
    for i in range(4):
        for byte in (1, 2):
            refused(ok, off=tuple(byte if j == i else 0 for j in range(4)), what='4-byte aligned')
    good = dict(gq.TINY_SIZES)
    for field, values in (('height', (4, 0, -8, 10, abi.RV_GQ_MAX_SIDE + 4)), ('width', (4, 9, abi.RV_GQ_MAX_SIDE + 4)),
                          ('c1', (0, 6, abi.RV_GQ_MAX_CHANNELS + 4)), ('c2', (0, -4, 5, abi.RV_GQ_MAX_CHANNELS + 4)),
                          ('f1', (0, 7, abi.RV_GQ_MAX_FEATURES + 4)), ('f2', (0, 6, abi.RV_GQ_MAX_FEATURES + 4)),
                          ('p', (0, 2, abi.RV_GQ_MAX_POSE + 4)), ('reserved', (1,))):
        for v in values:
            refused(abi.rv_grasp_quality_model(im_inv_std=1, z_inv_std=1, **dict(good, **{field: v})), what='outside its range')
    for field in gq.NORM_NAMES:
        for v in (float('nan'), float('inf'), float('-inf')):
            refused(abi.rv_grasp_quality_model(**dict(dict(good, im_inv_std=1, z_inv_std=1), **{field: v})), what='not finite')
    for k in (0, -1, abi.RV_AP_MAX_SAMPLES + 1):
        refused(ok, k=k, what='k outside')
    # the binding raises ValueError for them, and checks the shapes itself
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((1, abi.RV_AP_MAX_SAMPLES + 1, 8, 8), F), np.zeros((1, abi.RV_AP_MAX_SAMPLES + 1), F), m)
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((1, K, 8, 12), F), np.zeros((1, K), F), m)
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((2, K, 8, 8), F), np.zeros((2, K), F), m)
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((1, K, 8, 8), F), np.zeros((1, K + 1), F), m)
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((1, K, 8, 8), F), np.zeros((1, K), F), m, out=t.zeros((1, K + 1), device=world.device))
    bad = GraspQualityModel.random_init(0, norm=dict(NORM, z_mean=float('nan')), **good)
    with pytest.raises(ValueError):
        world.grasp_quality(np.zeros((1, K, 8, 8), F), np.zeros((1, K), F), bad)
    # the limits themselves run: K at RV_AP_MAX_SAMPLES (the tiny model), and the largest model the ranges allow
    kmax = abi.RV_AP_MAX_SAMPLES
    got = world.grasp_quality(x[None, :kmax], z[None, :kmax], m).cpu().numpy()[0]
    assert np.array_equal(_bits(got), _bits(want[:kmax]))
    big = GraspQualityModel.random_init(3, norm=NORM, height=abi.RV_GQ_MAX_SIDE, width=abi.RV_GQ_MAX_SIDE, c1=abi.RV_GQ_MAX_CHANNELS,
                                        c2=abi.RV_GQ_MAX_CHANNELS, f1=abi.RV_GQ_MAX_FEATURES, f2=abi.RV_GQ_MAX_FEATURES,
                                        p=abi.RV_GQ_MAX_POSE)
    xb, zb = gqh.sample_inputs(4, 3, abi.RV_GQ_MAX_SIDE, abi.RV_GQ_MAX_SIDE)
    got = world.grasp_quality(xb[None], zb[None], big).cpu().numpy()[0]
    assert np.array_equal(_bits(got), _bits(gqh.forward(big.params, big.norm, xb, zb)))


def _pose_only_model(**sizes):
    """logit = z * 4: only the pose stream, with a positive weight, reaches the output"""
    full = dict(gq.DEFAULT_SIZES, **sizes)
    m = GraspQualityModel({key: np.zeros(s, F) for key, s in gq.param_shapes(**full).items()},
                          dict(im_mean=0, im_inv_std=1, z_mean=0, z_inv_std=4), **full)
    m.params['pose.weight'][0, 0] = 1
    m.params['fc2.weight'][0, full['f1']] = 1
    m.params['out.weight'][0, 0] = 1
    return m


def test_env_level_logits_equal_the_separate_calls():
    from robovat_amd import envs
    n, K, seed = 4, 6, 5
    model = GraspQualityModel.random_init(8, norm=dict(im_mean=0.6, im_inv_std=8.0, z_mean=0.6, z_inv_std=20.0))
    small = GraspQualityModel.random_init(9, norm=NORM, **MODELS['8x12'])
    env = envs.VecGrasp4DofEnv(n, seed=seed)
    one = envs.Grasp4DofEnv(seed=seed)
    try:
        env.reset()
        with pytest.raises(ValueError):
            env.grasp_qualities(model)      # no sampling call before it
        env.sample_antipodal_candidates(K)
        before = env.world.save_state().blocks.cpu().numpy()
        for mdl, crop in ((model, {}), (small, dict(step=2))):
            got = env.grasp_qualities(mdl, **crop)
            assert tuple(got.shape) == (n, K)
            # the loop of separate calls
            d, _ = env.world.render()
            g = env.antipodal_image_grasps
            p = lib.grasp_crop_params(mdl.sizes['height'], mdl.sizes['width'], crop.get('step', 3))
            images, gd = env.world.grasp_crops(d, g, p)
            want = env.world.grasp_quality(images, gd, mdl)
            assert _same(got.cpu().numpy(), want.cpu().numpy()) and np.isfinite(want.cpu().numpy()).all()
            assert len(set(want.cpu().numpy().ravel().tolist())) > 1
            # explicit arguments
            assert _same(env.grasp_qualities(mdl, g[:, 0], d, **crop).cpu().numpy(), want.cpu().numpy()[:, :1])
            # and the kernel's logits are the restatement's on real crops
            host = gqh.forward(mdl.params, mdl.norm, images.cpu().numpy().reshape((n * K,) + tuple(images.shape[2:])), gd.cpu().numpy().ravel())
            assert _same(want.cpu().numpy(), host.reshape(n, K))
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        # Grasp4DofEnv (env 0 of the same seed): the vec env's row 0
        one.reset()
        with pytest.raises(ValueError):
            one.grasp_qualities(model)
        one._vec.sample_antipodal_candidates(K)      # (the vec form: an env without a grasp is not an error here)
        row = one.grasp_qualities(small, step=2)
        assert isinstance(row, np.ndarray) and _same(row, want.cpu().numpy()[0])
        assert _same(one.grasp_qualities(small, g[0, 1].cpu().numpy(), d[0].cpu().numpy(), step=2), want.cpu().numpy()[0, 1:2])
    finally:
        env.close()
        one.close()


@pytest.mark.parametrize('action_type', ['CUBOID', 'IMAGE'])
def test_policy_takes_the_highest_logit_among_the_valid_rows(action_type):
    from robovat_amd import envs, policies
    n, K, seed = 6, 8, 5
    model = _pose_only_model()
    cfg = configs.grasp_env_config(**{'ACTION.TYPE': action_type})
    env = envs.VecGrasp4DofEnv(n, config=cfg, seed=seed)
    one = envs.Grasp4DofEnv(config=configs.grasp_env_config(**{'ACTION.TYPE': action_type}), seed=seed)
    try:
        t = env.world.torch
        obs = env.reset()
        depth = obs['depth'].clone()
        depth[1] = depth[1].max()      # a flat image: no edge pixel, status != 1
        policy = policies.GraspQualityPolicy(env, model, K)
        before = env.world.save_state().blocks.cpu().numpy()
        a = policy.action({'depth': depth})
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        width = 4 if action_type == 'CUBOID' else 5
        assert tuple(a.shape) == (n, width) and tuple(policy.last_logits.shape) == (n, K) and tuple(policy.last_choice.shape) == (n,)
        st, cnt = env.antipodal_status.cpu().numpy(), env.antipodal_count.cpu().numpy()
        g = env.antipodal_image_grasps.cpu().numpy()
        logits, choice = policy.last_logits.cpu().numpy(), policy.last_choice.cpu().numpy()
        assert st[1] != 1 and (st == 1).sum() >= 2 and (cnt[st == 1] > 1).any()
        # the logit is 4 z exactly, so the choice is the deepest valid candidate, the lowest index among equals
        assert _same(logits, (g[:, :, 4] * F(4)).astype(F))
        assert _same(logits, env.grasp_qualities(model, depth=depth).cpu().numpy())
        for i in range(n):
            if st[i] != 1:
                assert choice[i] == 0
            else:
                zi = g[i, :cnt[i], 4]
                assert choice[i] == int(np.argmax(zi)) and zi[choice[i]] == zi.max()
        assert (choice > 0).any()
        cand = (env.antipodal_actions4 if action_type == 'CUBOID' else env.antipodal_image_grasps).cpu().numpy()
        assert _same(a.cpu().numpy(), cand[np.arange(n), choice])
        # a NaN among an env's valid logits: candidate 0
        nan_model = _pose_only_model()
        nan_model.params['out.bias'][0] = np.nan
        assert np.array_equal(policies.GraspQualityPolicy(env, nan_model, K).action({'depth': depth}).cpu().numpy().view(np.uint32),
                              cand[:, 0].view(np.uint32))
        # Grasp4DofEnv: row 0 of the vec env's
        obs1 = one.reset()
        p1 = policies.GraspQualityPolicy(one, model, K)
        assert st[0] == 1      # (seed 5: env 0 finds a grasp; without one the single env raises ValueError as its sampler does)
        a1 = p1.action({'depth': np.asarray(obs1['depth'])})
        assert isinstance(a1, np.ndarray) and _same(a1, a.cpu().numpy()[0])
        assert p1.last_choice == int(choice[0]) and _same(p1.last_logits, logits[0])
        # stepping with the returned actions works
        _, r, done, _ = env.step(a)
        assert tuple(r.shape) == (n,) and bool(t.isfinite(r).all())
        one.step(a1)
        with pytest.raises(ValueError):
            policies.GraspQualityPolicy(env, model, 0)
    finally:
        env.close()
        one.close()
