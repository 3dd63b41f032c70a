"""rv_grasp_refine on the MI355X: k_grasp_refine compared bit for bit with tests/grasp_refine_host.py (its
float32 NumPy restatement) on the synthetic images of tests/test_grasp_refine_host.py -- on a push world (stateless use) and
on a grasp world with actions4 --, its refusals, that no env state changes; then VecGrasp4DofEnv.refine_grasps on real
renders and CEMGraspPolicy.

What "bit for bit" covers: the rows, the parents and the counts, and the position [x, y, z] of actions4 (float32 sums,
products and quotients, restated exactly).  The yaw of actions4 goes through the device's libm (atan2f, cosf, sinf), whose
last bits no host restatement owns: it is compared within grasp_refine_host.YAW_TOL = 1e-5 rad (derived there; the tests
of rv_policy_antipodal_multi compare the same conversion within 1e-4), and bit for bit with rv_policy_antipodal_multi's own
actions wherever a row is a copy of one of that kernel's rows (test_refine_grasps_on_real_renders)."""
import ctypes as C

import numpy as np
import pytest

import grasp_refine_host as host
from robovat_amd import abi, configs, lib, scenes
from test_grasp_refine_host import SAMPLER, SAMPLER_CROP, SIGMAS, WORLD_SEED, H, W, synth_grasps, synth_images, synth_scores

pytestmark = pytest.mark.gpu
F = np.float32
POISON = -7.0
IPOISON = -77
SHAPES = [(1, 1), (2, 1), (5, 2), (9, 8), (64, 64), (64, 5)]      # (K, E)
KW = dict(macro_index=2, iteration=3, seed=0x9abcdef1)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _cfg(p):
    return {'SAMPLER': dict(p), 'GRIPPER_WIDTH': 0.038}


@pytest.fixture(scope='module')
def worlds():
    """push and grasp worlds of 1 env (global env id 2) and of 3; rv_grasp_refine takes N, the ids, the seed, the device
    and the stream from a world, and the calibration from a grasp world when actions4 are asked for"""
    out = {}
    scene, names = scenes.make_scene()
    gcfg = configs.grasp_env_config()
    gscene, gnames = scenes.make_scene(env_cfg=gcfg)
    for n, off in ((1, 2), (3, 0)):
        cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n,
                                     shape_names=names, seed=WORLD_SEED, env_id_offset=off)
        out['push', n] = lib.World(cfg, scene, device=0)
        out['grasp', n] = lib.World(configs.make_rv_config(env_cfg=gcfg, n_envs=n, seed=WORLD_SEED, shape_names=gnames,
                                                           env_id_offset=off), gscene, device=0)
        out['grasp', n].reset()
    yield out
    for w in out.values():
        w.close()


def _inputs(n, k):
    """images, parents, scores and (count, status) of a shape; env 0 keeps every row, the others show a short count and
    (N = 3) an env without a grasp"""
    img, g, s = synth_images(n), synth_grasps(n, k, seed=k), synth_scores(n, k, seed=k + 1)
    if k >= 5:
        g[0, 1] = [np.nan, 3, 4, 5, 0.6]      # a NaN row among the candidates
        s[0, 2] = np.inf
    count = np.array([k, max(k // 2, 1), k][:n], np.int32)
    status = np.array([1, 1, -2][:n], np.int32)
    return img, g, s, count, status


def _call(world, img, g, s, e, sigmas, sampler, count=None, status=None, actions4=False, lead=4, **kw):
    """rv_grasp_refine into buffers with guard words before and after: ``lead`` = 4: 16-byte aligned, 1: 4-byte aligned only"""
    t = world.torch
    n, k = g.shape[:2]
    dev = lambda a: None if a is None else t.as_tensor(np.ascontiguousarray(a), device=world.device)
    d_img, d_g, d_s, d_cnt, d_st = dev(img), dev(g), dev(s), dev(count), dev(status)
    sizes = {'g': n * k * 5, 'a': n * k * 4, 'p': n * k, 'c': n}
    bufs = {key: t.full((lead + size + 4,), POISON if key in 'ga' else IPOISON, dtype=t.float32 if key in 'ga' else t.int32,
                        device=world.device) for key, size in sizes.items()}
    view = {key: bufs[key][lead:lead + sizes[key]] for key in bufs}
    assert (view['g'].data_ptr() % 16 == 0) == (lead == 4)
    p = lib.grasp_refine_params(n_elites=e, sigma_center=sigmas[0], sigma_angle=sigmas[1], sigma_depth=sigmas[2], **kw)
    p.height, p.width = img.shape[1:]
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    sp = lib.antipodal_params(_cfg(sampler))
    rc = world.lib.rv_grasp_refine(world.h, C.byref(p), C.byref(sp), ptr(d_img), ptr(d_g), ptr(d_s), ptr(d_cnt), ptr(d_st), k,
                                   ptr(view['g']), ptr(view['a']) if actions4 else None, ptr(view['p']), ptr(view['c']))
    lib.check(rc)
    world.synchronize()
    for key, b in bufs.items():
        poison = POISON if key in 'ga' else IPOISON
        assert bool((b[:lead] == poison).all()) and bool((b[lead + sizes[key]:] == poison).all()), key
    if not actions4:
        assert bool((view['a'] == POISON).all())
    return (view['g'].cpu().numpy().reshape(n, k, 5), view['a'].cpu().numpy().reshape(n, k, 4) if actions4 else None,
            view['p'].cpu().numpy().reshape(n, k), view['c'].cpu().numpy())


def _check_actions(world, rows, a4):
    cam = world.camera().cpu().numpy()
    for n in range(rows.shape[0]):
        for j in range(rows.shape[1]):
            xyz, yaw = host.as_4dof(cam[n], rows[n, j])
            if np.isnan(xyz).any():      # (a NaN row: which NaN an operation returns is the hardware's business)
                assert np.array_equal(np.isnan(a4[n, j, :3]), np.isnan(xyz)), (n, j)
                continue
            assert np.array_equal(_bits(a4[n, j, :3]), _bits(xyz)), (n, j, a4[n, j], xyz)
            if np.isfinite(yaw):
                assert abs(np.angle(np.exp(1j * (float(a4[n, j, 3]) - yaw)))) <= host.YAW_TOL, (n, j, a4[n, j, 3], yaw)
            else:
                assert np.isnan(a4[n, j, 3])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('k,e', SHAPES)
def test_kernel_equals_the_host_restatement(worlds, k, e, n):
    img, g, s, count, status = _inputs(n, k)
    off = 2 if n == 1 else 0
    fallbacks = children = 0
    for sampler, sigmas in ((SAMPLER, SIGMAS), (SAMPLER_CROP, (9.0, 0.4, 0.02))):
        for cs in ((None, None), (count, status)):
            want_g, want_p, want_c = host.refine(img, g, s, e, sigmas, sampler, count=cs[0], status=cs[1],
                                                 world_seed=WORLD_SEED, env_id_offset=off, **KW)
            fallbacks += int((want_p < 0).sum()); children += int((want_p[:, e:] >= 0).sum())
            for kind, lead in (('push', 4), ('push', 1), ('grasp', 4), ('grasp', 1)):
                world = worlds[kind, n]
                got_g, got_a, got_p, got_c = _call(world, img, g, s, e, sigmas, sampler, count=cs[0], status=cs[1],
                                                   actions4=kind == 'grasp', lead=lead, **KW)
                differ = int((_bits(got_g) != _bits(want_g)).sum())
                print('K = %d E = %d N = %d %s lead %d: %d of %d floats differ from the restatement' % (k, e, n, kind, lead, differ, want_g.size))
                assert differ == 0
                assert np.array_equal(got_p, want_p) and np.array_equal(got_c, want_c)
                if kind == 'grasp' and lead == 4:
                    _check_actions(world, got_g, got_a)
    if k == 64 and e == 5:
        assert fallbacks > 10 and children > 100      # both outcomes were compared


def test_refusals_leave_poisoned_outputs_untouched(worlds):
    world, push = worlds['grasp', 3], worlds['push', 3]
    t = world.torch
    n, k = 3, 6
    img, g, s, count, status = _inputs(n, k)
    dev = lambda a: t.as_tensor(np.ascontiguousarray(a), device=world.device)
    d = {'depth': dev(np.concatenate([img.ravel(), np.zeros(4, F)])), 'grasps': dev(np.concatenate([g.ravel(), np.zeros(4, F)])),
         'scores': dev(np.concatenate([s.ravel(), np.zeros(4, F)])), 'count': dev(np.concatenate([count, np.zeros(4, np.int32)])),
         'status': dev(np.concatenate([status, np.zeros(4, np.int32)]))}
    outs = {'g': t.full((n * 64 * 5 + 8,), POISON, dtype=t.float32, device=world.device),
            'a': t.full((n * 64 * 4 + 8,), POISON, dtype=t.float32, device=world.device),
            'p': t.full((n * 64 + 8,), IPOISON, dtype=t.int32, device=world.device),
            'c': t.full((n + 8,), IPOISON, dtype=t.int32, device=world.device)}
    ptr = lambda v, off=0: None if v is None else C.c_void_p(v.data_ptr() + off)
    good_p = lambda **kw: lib.grasp_refine_params(**dict(dict(n_elites=2, height=H, width=W), **kw))
    good_s = lib.antipodal_params(_cfg(SAMPLER))

    def refused(what, w=world, p=None, sp=good_s, k=k, null=(), off=None, alias=False, no_params=False, no_sampler=False):
        p = good_p() if p is None else p
        o = dict(off or {})
        a = {key: (None if key in null else ptr(v, o.get(key, 0))) for key, v in list(d.items()) + list(outs.items())}
        if alias:
            a['g'] = a['grasps']
        rc = w.lib.rv_grasp_refine(w.h, None if no_params else C.byref(p), None if no_sampler else C.byref(sp), a['depth'],
                                   a['grasps'], a['scores'], a['count'], a['status'], k, a['g'], a['a'], a['p'], a['c'])
        assert rc == abi.RV_ERR_VALUE and what.encode() in w.lib.rv_last_error(), (what, rc, w.lib.rv_last_error())
        w.synchronize()
        for key, b in outs.items():
            assert bool((b == (POISON if key in 'ga' else IPOISON)).all()), (what, key)
        if alias:
            assert np.array_equal(_bits(d['grasps'].cpu().numpy()[:g.size]), _bits(g.ravel()))

    refused('null params', no_params=True); refused('null params', no_sampler=True)
    for key in ('depth', 'grasps', 'scores', 'g'):
        refused('null buffer', null=(key,))
    for key in list(d) + list(outs):
        for byte in (1, 2):
            refused('4-byte aligned', off={key: byte})
    refused('must not be d_grasps', alias=True)
    for kk in (0, -1, abi.RV_AP_MAX_SAMPLES + 1):
        refused('k outside', k=kk)
    for e in (0, -1, k + 1):
        refused('n_elites outside', p=good_p(n_elites=e))
    refused('height or width', p=good_p(height=0)); refused('height or width', p=good_p(width=-3))
    for field in ('sigma_center', 'sigma_angle', 'sigma_depth'):
        for v in (-1e-3, float('nan'), float('inf'), float('-inf')):
            refused('sigma', p=good_p(**{field: v}))
    refused('macro_index outside', p=good_p(macro_index=-1)); refused('macro_index outside', p=good_p(macro_index=abi.RV_GR_MAX_MACRO_INDEX))
    refused('iteration outside', p=good_p(iteration=-1)); refused('iteration outside', p=good_p(iteration=abi.RV_GR_MAX_ITERATION))
    for i in range(3):
        p = good_p(); p.reserved[i] = 1
        refused('reserved', p=p)
    # what rv_policy_antipodal_multi refuses of the sampler's parameters
    for change, what in ((dict(MIN_DIST_FROM_BOUNDARY=2), 'MIN_DIST_FROM_BOUNDARY'), (dict(DEPTH_SAMPLE_WINDOW_WIDTH=0.5), 'MIN_DIST_FROM_BOUNDARY'),
                         (dict(CROP=[0, 0, H + 1, W]), 'CROP'), (dict(CROP=[10, 5, 10, 20]), 'CROP'), (dict(DOWNSAMPLE_RATE=9), 'DOWNSAMPLE_RATE'),
                         (dict(DEPTH_SAMPLES_PER_GRASP=2), 'DEPTH_SAMPLES_PER_GRASP'), (dict(MAX_REJECTION_SAMPLES=0), 'MAX_REJECTION_SAMPLES')):
        refused(what, sp=lib.antipodal_params(_cfg(dict(SAMPLER, **change))))
    refused('needs a Grasp4DofEnv world', w=push)
    # the limits run: the largest macro_index and iteration, and the binding raises ValueError for a refusal
    last = good_p(macro_index=abi.RV_GR_MAX_MACRO_INDEX - 1, iteration=abi.RV_GR_MAX_ITERATION - 1)
    got = world.grasp_refine(img, g, s, last, good_s)[0].cpu().numpy()
    want = host.refine(img, g, s, 2, (3.0, 0.15, 0.005), SAMPLER, world_seed=WORLD_SEED,
                       macro_index=abi.RV_GR_MAX_MACRO_INDEX - 1, iteration=abi.RV_GR_MAX_ITERATION - 1)[0]
    assert np.array_equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):
        world.grasp_refine(img, g, s, good_p(n_elites=k + 1), good_s)
    with pytest.raises(ValueError):
        push.grasp_refine(img, g, s, good_p(), good_s, actions4=True)
    with pytest.raises(ValueError):
        world.grasp_refine(img, g, s[:, :3], good_p(), good_s)
    with pytest.raises(TypeError):
        lib.grasp_refine_params(nonsense=1)


def test_no_env_state_changes(worlds):
    for kind in ('push', 'grasp'):
        world = worlds[kind, 3]
        img, g, s, count, status = _inputs(3, 9)
        before = world.save_state().blocks.cpu().numpy()
        out = world.grasp_refine(img, g, s, lib.grasp_refine_params(n_elites=3), lib.antipodal_params(_cfg(SAMPLER)),
                                 count=count, status=status, actions4=kind == 'grasp')
        world.synchronize()
        assert (out[1] is None) == (kind == 'push') and tuple(out[0].shape) == (3, 9, 5)
        assert np.array_equal(world.save_state().blocks.cpu().numpy(), before)


def _tiny_model(seed=4):
    from robovat_amd.perception import grasp_quality as gq
    return gq.GraspQualityModel.random_init(seed, norm=dict(im_mean=0.6, im_inv_std=8.0, z_mean=0.6, z_inv_std=20.0), **gq.TINY_SIZES)


def test_refine_grasps_on_real_renders():
    """VecGrasp4DofEnv.refine_grasps == the separate World.grasp_refine call == the restatement, on renders of 8 config-4
    grasp envs; rows copied from the sampler's carry the sampler's own actions bit for bit; Grasp4DofEnv is row 0"""
    from robovat_amd import envs
    n, K, seed = 8, 8, 5
    env = envs.VecGrasp4DofEnv(n, seed=seed)
    one = envs.Grasp4DofEnv(seed=seed)
    try:
        env.reset()
        with pytest.raises(ValueError):
            env.refine_grasps(np.zeros((n, K), F), 2, SIGMAS, 0)      # no sampling call before it
        depth, _ = env.world.render()
        env.sample_antipodal_candidates(K, depth=depth)
        g0, a0 = env.antipodal_image_grasps.clone(), env.antipodal_actions4.clone()
        cnt0, st0 = env.antipodal_count.clone(), env.antipodal_status.clone()
        scores = env.grasp_qualities(_tiny_model(), depth=depth)
        before = env.world.save_state().blocks.cpu().numpy()
        sig = (3.0, 0.15, 0.005)
        params = lib.grasp_refine_params(n_elites=3, sigma_center=sig[0], sigma_angle=sig[1], sigma_depth=sig[2],
                                         macro_index=0, iteration=1, seed=9)
        wg, wa, wp, wc = env.world.grasp_refine(depth, g0, scores, params, lib.antipodal_params(), count=cnt0, status=st0, actions4=True)
        ret = env.refine_grasps(scores, 3, sig, 1, depth=depth, seed=9)
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        assert ret is env.antipodal_actions4
        for got, want in ((env.antipodal_image_grasps, wg), (env.antipodal_actions4, wa), (env.refine_parent, wp), (env.antipodal_count, wc)):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        # ... == the restatement, with the policy config's sampler parameters and crop
        hg, hp, hc = host.refine(depth.cpu().numpy(), g0.cpu().numpy(), scores.cpu().numpy(), 3, sig,
                                 configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG['SAMPLER'], count=cnt0.cpu().numpy(),
                                 status=st0.cpu().numpy(), world_seed=seed, macro_index=0, iteration=1, seed=9)
        assert np.array_equal(_bits(wg.cpu().numpy()), _bits(hg)) and np.array_equal(wp.cpu().numpy(), hp)
        assert np.array_equal(wc.cpu().numpy(), hc)
        st, par = st0.cpu().numpy(), hp
        assert (st == 1).sum() >= 4 and (par[st == 1][:, 3:] >= 0).any()
        # a row that is a copy of a sampler row carries that kernel's action, bit for bit
        a0n, wan = a0.cpu().numpy(), wa.cpu().numpy()
        copies = 0
        cnt = cnt0.cpu().numpy()
        for i in range(n):
            for j in range(K):
                src = par[i, j] if (st[i] != 1 or j < min(3, cnt[i])) else (-1 - par[i, j] if par[i, j] < 0 else None)
                if src is not None:
                    assert np.array_equal(_bits(wan[i, j]), _bits(a0n[i, src])), (i, j)
                    copies += 1
        assert copies >= sum(min(3, c) for c in cnt.tolist()) >= 12
        _check_actions(env.world, wg.cpu().numpy(), wan)
        # the depth is rendered when it is not given, and a second round takes the first round's rows
        env.sample_antipodal_candidates(K, depth=depth)
        env.refine_grasps(scores, 3, sig, 1, seed=9)
        assert np.array_equal(_bits(env.antipodal_image_grasps.cpu().numpy()), _bits(hg))
        s2 = env.grasp_qualities(_tiny_model(), depth=depth)
        env.refine_grasps(s2, 2, sig, 2, depth=depth, seed=9)
        h2 = host.refine(depth.cpu().numpy(), hg, s2.cpu().numpy(), 2, sig, configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG['SAMPLER'],
                         count=hc, status=st, world_seed=seed, macro_index=0, iteration=2, seed=9)
        assert np.array_equal(_bits(env.antipodal_image_grasps.cpu().numpy()), _bits(h2[0]))
        assert np.array_equal(env.refine_parent.cpu().numpy(), h2[1])
        # Grasp4DofEnv (env 0 of the same seed): the vec env's row 0
        one.reset()
        one._vec.sample_antipodal_candidates(K)
        row = one.refine_grasps(scores[0].cpu().numpy(), 3, sig, 1, seed=9)
        assert isinstance(row, np.ndarray) and np.array_equal(_bits(row), _bits(wan[0]))
        assert np.array_equal(one.refine_parent.cpu().numpy()[0], hp[0])
    finally:
        env.close()
        one.close()


@pytest.mark.parametrize('action_type', ['CUBOID', 'IMAGE'])
def test_cem_grasp_policy(action_type):
    from robovat_amd import envs, policies
    n, K, seed = 8, 8, 5
    model = _tiny_model()
    cfg = configs.grasp_env_config(**{'ACTION.TYPE': action_type})
    env = envs.VecGrasp4DofEnv(n, config=cfg, seed=seed)
    one = envs.Grasp4DofEnv(config=configs.grasp_env_config(**{'ACTION.TYPE': action_type}), seed=seed)
    try:
        obs = env.reset()
        depth = obs['depth'].clone()
        depth[1] = depth[1].max()      # a flat image: no edge pixel, an env without a grasp
        width = 4 if action_type == 'CUBOID' else 5
        before = env.world.save_state().blocks.cpu().numpy()
        policy = policies.CEMGraspPolicy(env, K, num_iterations=2, model=model, seed=3)
        assert policy.num_elites == 2
        a = policy.action({'depth': depth})
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        assert tuple(a.shape) == (n, width)
        assert len(policy.last_scores) == 3 and all(tuple(s.shape) == (n, K) for s in policy.last_scores)
        assert len(policy.last_choice_parentage) == 3 and tuple(policy.last_grasps.shape) == (n, K, 5)
        st = env.antipodal_status.cpu().numpy()
        assert st[1] != 1 and (st == 1).sum() >= 4
        # the best score of an env never goes down from one scoring to the next: exact, the elites are copies
        sc = [s.cpu().numpy() for s in policy.last_scores]
        assert all(np.isfinite(s).all() for s in sc)
        for t in range(2):
            assert np.all(sc[t + 1].max(axis=1) >= sc[t].max(axis=1)), t
        print('%s: envs whose best score rose: %s' % (action_type, [int((sc[t + 1].max(axis=1) > sc[t].max(axis=1)).sum()) for t in range(2)]))
        # row 0 of the sorted final rows is the action, and carries the last scoring's best
        cand = (env.antipodal_actions4 if action_type == 'CUBOID' else env.antipodal_image_grasps).cpu().numpy()
        final_parent = policy.last_choice_parentage[-1].cpu().numpy()
        for i in range(n):
            if st[i] == 1:
                assert np.array_equal(_bits(a.cpu().numpy()[i]), _bits(cand[i, 0]))
                assert sc[2][i, final_parent[i, 0]] == sc[2][i].max()
        # num_iterations = 0 is GraspQualityPolicy, bit for bit; the env without a grasp takes candidate 0 of the sampling
        gq_action = policies.GraspQualityPolicy(env, model, K).action({'depth': depth}).cpu().numpy()
        first = (env.antipodal_actions4 if action_type == 'CUBOID' else env.antipodal_image_grasps).cpu().numpy()[:, 0].copy()
        zero = policies.CEMGraspPolicy(env, K, num_iterations=0, model=model).action({'depth': depth}).cpu().numpy()
        assert np.array_equal(_bits(zero), _bits(gq_action))
        assert np.array_equal(_bits(a.cpu().numpy()[1]), _bits(first[1])) and np.array_equal(_bits(zero[1]), _bits(first[1]))
        # scores that are all NaN: candidate 0 in every env
        nan_model = _tiny_model()
        nan_model.params['out.bias'][0] = np.nan
        got = policies.CEMGraspPolicy(env, K, num_iterations=2, model=nan_model).action({'depth': depth}).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(first))
        # the simulator as the scorer: the chosen action earns at least the best reward of the initial candidates
        sim = policies.CEMGraspPolicy(env, K, num_iterations=2, score='simulator', seed=3)
        a_sim = sim.action({'depth': depth})
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        r0 = sim.last_scores[0].cpu().numpy()
        a4 = env.antipodal_actions4[:, :1].clone()      # (row 0 of the sorted final rows, with the env's own calibration)
        chosen, _ = env.try_grasps(a4)
        chosen = chosen.cpu().numpy()[:, 0]
        for i in range(n):
            if st[i] == 1:
                assert chosen[i] >= r0[i].max(), (i, chosen[i], r0[i])
                assert np.array_equal(_bits(a_sim.cpu().numpy()[i]), _bits((env.antipodal_actions4 if action_type == 'CUBOID' else env.antipodal_image_grasps).cpu().numpy()[i, 0]))
        rs = [s.cpu().numpy() for s in sim.last_scores]
        assert all(np.all(rs[t + 1].max(axis=1) >= rs[t].max(axis=1)) for t in range(2))
        # Grasp4DofEnv: row 0 of the vec env's
        obs1 = one.reset()
        assert st[0] == 1
        p1 = policies.CEMGraspPolicy(one, K, num_iterations=2, model=model, seed=3)
        a1 = p1.action({'depth': np.asarray(obs1['depth'])})
        assert isinstance(a1, np.ndarray) and np.array_equal(_bits(a1), _bits(a.cpu().numpy()[0]))
        # stepping with the returned actions works
        _, r, done, _ = env.step(a)
        assert tuple(r.shape) == (n,) and bool(env.world.torch.isfinite(r).all())
        one.step(a1)
        for bad in (dict(num_samples=0), dict(num_samples=K, num_iterations=-1), dict(num_samples=K, num_elites=K + 1),
                    dict(num_samples=K, score='oracle'), dict(num_samples=K, model=None)):
            with pytest.raises(ValueError):
                policies.CEMGraspPolicy(env, **dict(dict(model=model), **bad))
    finally:
        env.close()
        one.close()
