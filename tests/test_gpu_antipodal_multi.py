"""rv_policy_antipodal_multi on the MI355X: K grasps per env against the NumPy restatement (tests/antipodal_multi_host.py)
on the reference's golden images and on the oracle's renders, its parameter checks, and what is built on it:
VecGrasp4DofEnv.try_grasps / save_state / restore_state and LookaheadGrasp4DofPolicy."""
import copy
import json
import os

import numpy as np
import pytest

import antipodal_host as host
import antipodal_multi_host as multi
from robovat_amd import abi, configs, scenes
from test_gpu_antipodal import NOISE, _camera, _policy_params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N = 8

with open(os.path.join(HERE, 'golden', 'antipodal_multi_golden.json')) as _f:
    GOLDEN = json.load(_f)
with open(os.path.join(HERE, 'golden', 'antipodal_golden.json')) as _f:
    SPECS = {c['name']: c['spec'] for c in json.load(_f)['cases']}
CASE_NAMES = sorted({c['name'] for c in GOLDEN['cases']})


def _world(image, n=N):
    from robovat_amd import lib
    h_, w_ = image.shape
    env_cfg = configs.grasp_env_config(**{'KINECT2.DEPTH.HEIGHT': h_, 'KINECT2.DEPTH.WIDTH': w_,
                                          'KINECT2.DEPTH.INTRINSICS': GOLDEN['intrinsics']})
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    world = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=GOLDEN['seed'], shape_names=names), scene, device=0)
    world.reset()
    return world


def _cfg(p):
    return {'SAMPLER': {k: v for k, v in p.items() if k != 'GRIPPER_WIDTH'}, 'GRIPPER_WIDTH': p['GRIPPER_WIDTH']}


def _check_rows(what, g, a4, cnt, st, h, cam_row, rnd_row):
    """one env's rows [K, 5], [K, 4] against its restatement ``h``; returns False when they differ in status, count or pixels"""
    from robovat_amd.envs.grasp.grasp_2d import Grasp2D
    K = len(g)
    if st != h['status'] or cnt != h['count'] or (h['status'] == 1 and not np.array_equal(g[:, :4], h['grasps'][:, :4])):
        return False
    camera = _camera(cam_row)
    if st == 1:
        assert np.all(np.abs(g[:, 4] - h['grasps'][:, 4]) <= 1e-6 * np.abs(h['grasps'][:, 4])), what
        for k in range(cnt, K):
            assert np.array_equal(g[k].view(np.uint32), g[0].view(np.uint32)) and np.array_equal(a4[k].view(np.uint32), a4[0].view(np.uint32)), what
        for k in range(cnt):
            want = np.array(Grasp2D.from_vector(g[k], camera=camera).as_4dof())
            assert np.allclose(a4[k, :3], want[:3], atol=1e-4), (what, k, a4[k], want)
            assert abs(np.angle(np.exp(1j * (a4[k, 3] - want[3])))) < 1e-4, (what, k)
    else:
        assert cnt == 0, what
        for k in range(K):
            assert np.array_equal(a4[k], rnd_row), (what, k)
            assert np.array_equal(g[k].view(np.uint32), g[0].view(np.uint32)), (what, k)
        back = np.array(Grasp2D.from_vector(g[0], camera=camera).as_4dof())
        assert np.allclose(back[:3], rnd_row[:3], atol=1e-4), what
    return True


def _run_case(case_list, world, image, bases):
    from robovat_amd import lib
    K3 = GOLDEN['intrinsics']
    n = world.n
    depth = np.broadcast_to(image, (n,) + image.shape).copy()
    cam = world.camera().cpu().numpy()
    rnd = world.policy_random(0).cpu().numpy()[:, 0]
    out = {}
    for case in case_list:
        p, K = case['params'], case['num_samples']
        g, a4, cnt, st = world.policy_antipodal_multi(lib.antipodal_params(_cfg(p)), 0, K, depth=depth)
        g, a4, cnt, st = g.cpu().numpy(), a4.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy()
        assert g.shape == (n, K, 5) and a4.shape == (n, K, 4)
        hs = []
        for e in case['gids']:
            i = e['gid']
            key = (case['name'], json.dumps(p, sort_keys=True), i)
            if key not in bases:
                bases[key] = host.sample(image, p, K3[0][0], K3[0][2], seed=GOLDEN['seed'], gid=i, macro_index=0)
            h = multi.sample_multi(image, p, K3[0][0], K3[0][2], K, seed=GOLDEN['seed'], gid=i, macro_index=0, base=bases[key])
            hs.append(h)
            what = (case['name'], K, i)
            same = _check_rows(what, g[i], a4[i], int(cnt[i]), int(st[i]), h, cam[i], rnd[i])
            # (the golden marks the env ids where float32 and the reference's float64 decide a cone test differently:
            # the only ones excused)
            assert same or e.get('borderline'), (what, st[i], h['status'], cnt[i], h['count'], g[i], h['grasps'])
            if same and not e.get('borderline') and e['rows'] is not None:
                assert np.array_equal(g[i, :, :4], np.array(e['rows'])[:, :4]), what      # == the reference itself
        if K == 1:
            g1, a1, s1 = world.policy_antipodal(lib.antipodal_params(_cfg(p)), 0, depth=depth)
            assert np.array_equal(g1.cpu().numpy().view(np.uint32), g[:, 0].view(np.uint32)), case['name']
            assert np.array_equal(a1.cpu().numpy().view(np.uint32), a4[:, 0].view(np.uint32)), case['name']
            assert np.array_equal(s1.cpu().numpy(), st), case['name']
        out[K] = (hs, cnt, st)
    return out


@pytest.mark.parametrize('name', CASE_NAMES)
def test_golden_images_k_1_4_16(name):
    """(a) 8 envs on one golden image, K in {1, 4, 16}: status, count and pixels equal the restatement (and, off the env
    ids the golden marks as borderline, the reference's own rows), depth to 1e-6 relative, actions4 ==
    Grasp2D.from_vector(...).as_4dof(); K = 1 is rv_policy_antipodal bit for bit."""
    cases = [c for c in GOLDEN['cases'] if c['name'] == name]
    assert sorted(c['num_samples'] for c in cases) == [1, 4, 16]
    image = host.synth_image(SPECS[name])
    world = _world(image)
    try:
        _run_case(cases, world, image, {})
    finally:
        world.close()


def test_long_walk_nan_distance_and_nothing_accepted():
    """(b) wide_gripper0 at MIN_GRASP_DIST 12, K 16 (all 4000 draws walked: more than one key window); two_r3 at
    MIN_GRASP_DIST 1e6 (a second grasp only through a NaN distance); zero_bg_r2 (7856 valid pairs, none passes)."""
    for case in GOLDEN['extra']:
        image = host.synth_image(SPECS[case['name']])
        world = _world(image)
        try:
            hs, cnt, st = _run_case([case], world, image, {})[case['num_samples']]
        finally:
            world.close()
        if case['name'] == 'wide_gripper0':
            # the walk goes past half the selection buffer (RV_AP_SEL / 2 = 1024 pairs, the size a key window aims at) in
            # a set of valid pairs larger than the buffer: the first window cannot hold it all
            assert any(h['walked'] > 1024 and len(h['base']['valid_idx'][0]) > 2048 for h in hs)
            assert all(2 <= c <= 4 for c in cnt)
        elif case['name'] == 'two_r3':
            assert case['params']['MIN_GRASP_DIST'] == 1e6 and (cnt == 2).any() and (cnt <= 2).all()
        else:
            assert (st == abi.RV_AP_ALL_REJECTED).all() and (cnt == 0).all()
            assert all(len(h['base']['valid_idx'][0]) == 7856 for h in hs)


def test_config4_renders_k8_against_the_restatement():
    """(c) 64 config-4 envs with camera noise, K = 8, on the oracle's renders of the same envs."""
    from robovat_amd import lib
    from oracle import orc
    env_cfg = configs.grasp_env_config(**NOISE)
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    seed, m, K = 21, 3, 8
    cfg = configs.make_rv_config(env_cfg=env_cfg, n_envs=64, seed=seed, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    ref = orc.OracleWorld(cfg, scene, double=False)
    world.reset(); ref.reset()
    g, a4, cnt, st = world.policy_antipodal_multi(lib.antipodal_params(), m, K)
    g, a4, cnt, st = g.cpu().numpy(), a4.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy()
    cam = world.camera().cpu().numpy()
    rnd = world.policy_random(m).cpu().numpy()[:, 0]
    world.close()
    P = _policy_params()
    excused, several = [], 0
    for i in range(64):
        depth, _ = ref.render(i)
        h = multi.sample_multi(depth, P, cam[i, 0], cam[i, 2], K, seed=seed, gid=i, macro_index=m)
        if not _check_rows(('config4', i), g[i], a4[i], int(cnt[i]), int(st[i]), h, cam[i], rnd[i]):
            assert h['borderline'], (i, st[i], h['status'], cnt[i], h['count'], g[i], h['grasps'])
            excused.append(i)
            continue
        several += h['count'] >= 2
    print('antipodal multi vs restatement: %d / 64 envs with >= 2 grasps, excused %s, counts %s' % (several, excused, np.bincount(cnt, minlength=K + 1)))
    assert len(excused) <= 4
    assert several >= 40


def test_invalid_arguments_raise_value_error():
    """(d) what rv_policy_antipodal refuses, a K outside [1, RV_AP_MAX_SAMPLES], a NULL d_count, a push world."""
    import ctypes as C
    from robovat_amd import lib
    env_cfg = configs.grasp_env_config()
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    world = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=4, seed=1, shape_names=names), scene, device=0)
    world.reset()
    bad = [('DEPTH_SAMPLES_PER_GRASP', 2), ('DOWNSAMPLE_RATE', 9), ('DOWNSAMPLE_RATE', 1.5), ('MIN_DIST_FROM_BOUNDARY', 2),
           ('DEPTH_SAMPLE_WINDOW_HEIGHT', 0.5), ('CROP', [0, 0, 500, 100]), ('DEPTH_GRAD_GAUSSIAN_SIGMA', 9.0),
           ('MAX_REJECTION_SAMPLES', 0)]
    for key, value in bad:
        cfg = copy.deepcopy(configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG)
        cfg['SAMPLER'][key] = value
        with pytest.raises(ValueError) as e:
            world.policy_antipodal_multi(lib.antipodal_params(cfg), 0, 4)
        assert 'rv_policy_antipodal_multi' in str(e.value), key
    for k in (0, -1, abi.RV_AP_MAX_SAMPLES + 1):
        with pytest.raises(ValueError) as e:
            world.policy_antipodal_multi(lib.antipodal_params(), 0, k)
        assert 'rv_policy_antipodal_multi' in str(e.value) and 'num_samples' in str(e.value)
    world.policy_antipodal_multi(lib.antipodal_params(), 0, abi.RV_AP_MAX_SAMPLES)      # (the largest K runs)
    t = world.torch
    g = t.zeros((4, 2, 5), dtype=t.float32, device=world.device)
    st = t.full((4,), 77, dtype=t.int32, device=world.device)
    p = lib.antipodal_params()
    rc = world.lib.rv_policy_antipodal_multi(world.h, None, C.byref(p), 0, 2, C.c_void_p(g.data_ptr()), None, None, C.c_void_p(st.data_ptr()))
    assert rc == abi.RV_ERR_VALUE and b'rv_policy_antipodal_multi' in world.lib.rv_last_error()
    world.synchronize()
    assert (st == 77).all() and (g == 0).all()      # nothing was launched
    world.close()
    push_scene, push_names = scenes.make_scene()
    push = lib.World(configs.make_rv_config(n_envs=2, shape_names=push_names), push_scene, device=0)
    with pytest.raises(ValueError) as e:
        push.policy_antipodal_multi(lib.antipodal_params(), 0, 4)
    assert 'rv_policy_antipodal_multi' in str(e.value)
    push.close()


def test_try_grasps_equals_stepping_each_candidate_and_leaves_the_env_alone():
    """(e) N = 4, K = 3, candidate 1 aimed at the object: rewards and dones equal the float oracle stepping each candidate
    straight through from the same reset; the env's state bytes do not change; restore_state + step == the first step."""
    from robovat_amd import envs
    from oracle import orc
    n, K, seed = 4, 3, 5
    env = envs.VecGrasp4DofEnv(n, seed=seed)
    try:
        env.reset()
        acts = np.stack([env.world.policy_random(k).cpu().numpy()[:, 0] for k in range(K)], axis=1)      # [N, K, 4]
        acts[:, 1, :2] = env.world.body_state().cpu().numpy()[:, 0, :2]
        before = env.world.save_state().blocks.cpu().numpy()
        r, d = env.try_grasps(acts)
        assert tuple(r.shape) == (n, K) and tuple(d.shape) == (n, K) and str(r.dtype) == 'torch.float32' and str(d.dtype) == 'torch.uint8'
        r, d = r.cpu().numpy(), d.cpu().numpy()
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before)
        for k in range(K):
            ref = orc.OracleWorld(env.rv_config, env.scene, double=False)
            ref.reset()
            ref.set_actions(acts[:, k][:, None])
            ref.step_macro()
            rr, rd = ref.reward()
            assert np.array_equal(r[:, k].view(np.uint32), rr.astype(np.float32).view(np.uint32)), k
            assert np.array_equal(d[:, k] != 0, np.asarray(rd) != 0), k
        assert d.all()      # (a grasp episode is one step)
        # a second call on the kept plan world gives the same
        r2, d2 = env.try_grasps(acts)
        assert np.array_equal(r2.cpu().numpy().view(np.uint32), r.view(np.uint32)) and np.array_equal(d2.cpu().numpy(), d)
        snap = env.save_state()
        _, r_a, d_a, _ = env.step(acts[:, 1])
        after = env.world.save_state().blocks.cpu().numpy()
        assert not np.array_equal(after, before)
        assert np.array_equal(r_a.cpu().numpy().view(np.uint32), r[:, 1].view(np.uint32))
        env.restore_state(snap)
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), before) and env._macro_index == 0
        _, r_b, d_b, _ = env.step(acts[:, 1])
        assert np.array_equal(env.world.save_state().blocks.cpu().numpy(), after)
        assert np.array_equal(r_b.cpu().numpy().view(np.uint32), r_a.cpu().numpy().view(np.uint32)) and bool((d_a == d_b).all())
        with pytest.raises(ValueError):
            env.try_grasps(acts[:, :, :3])
    finally:
        env.close()


def test_lookahead_policy_never_does_worse_than_the_one_grasp_policy():
    """(f) 64 envs, K = 4: the reward of env.step(chosen) is the reward try_grasps saw, bit for bit; env by env the
    look-ahead succeeds wherever the one-grasp policy does (candidate 0 is its grasp); two runs give the same actions."""
    from robovat_amd import envs, policies
    n, K, seed, steps = 64, 4, 9, 2
    runs = []
    for _ in range(2):
        env = envs.VecGrasp4DofEnv(n, seed=seed)
        policy = policies.LookaheadGrasp4DofPolicy(env, K)
        acts, rewards, firsts = [], [], []
        try:
            for step in range(steps):
                obs = env.reset()
                a = policy.action(obs)
                assert tuple(a.shape) == (n, 4) and tuple(policy.last_rewards.shape) == (n, K) and tuple(policy.last_choice.shape) == (n,)
                seen = policy.last_rewards.cpu().numpy()
                choice = policy.last_choice.cpu().numpy()
                assert np.array_equal(a.cpu().numpy(), env.antipodal_actions4.cpu().numpy()[np.arange(n), choice])
                want = np.where((seen > 0).any(1), (seen > 0).argmax(1), 0)
                assert np.array_equal(choice, want)
                _, r, _, _ = env.step(a)
                r = r.cpu().numpy()
                assert np.array_equal(r.view(np.uint32), seen[np.arange(n), choice].view(np.uint32)), step
                acts.append(a.cpu().numpy()); rewards.append(r); firsts.append(env.antipodal_actions4.cpu().numpy()[:, 0])
        finally:
            env.close()
        runs.append((np.stack(acts), np.stack(rewards), np.stack(firsts)))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    env = envs.VecGrasp4DofEnv(n, seed=seed)
    policy = policies.AntipodalGrasp4DofPolicy(env)
    try:
        for step in range(steps):
            obs = env.reset()
            a = policy.action(obs)
            assert np.array_equal(a.cpu().numpy().view(np.uint32), runs[0][2][step].view(np.uint32))      # candidate 0
            _, r, _, _ = env.step(a)
            r = r.cpu().numpy()
            assert ((runs[0][1][step] > 0) >= (r > 0)).all(), step
            print('step %d: success one grasp %.3f, look-ahead K = %d %.3f' % (step, (r > 0).mean(), K, (runs[0][1][step] > 0).mean()))
    finally:
        env.close()
