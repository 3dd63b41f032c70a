"""AntipodalGrasp4DofPolicy on the MI355X (rv_policy_antipodal): against the NumPy restatement on the oracle's renders,
against the reference's own sampler on the golden synthetic images, end to end, and its parameter checks."""
import base64
import json
import os
import zlib

import numpy as np
import pytest

import antipodal_host as host
from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NOISE = {'KINECT2.DEPTH.INTRINSICS_NOISE': [[4.0, 0.0, 3.0], [0.0, 4.0, 3.0], [0.0, 0.0, 0.0]],
         'KINECT2.DEPTH.TRANSLATION_NOISE': [0.004, 0.004, 0.004],
         'KINECT2.DEPTH.ROTATION_NOISE': [[0.003] * 3] * 3}


def _policy_params(config=None):
    c = config or configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG
    p = dict(c['SAMPLER'])
    p['GRIPPER_WIDTH'] = c['GRIPPER_WIDTH']
    return p


def _camera(row):
    from robovat_amd.perception import Camera
    fx, fy, cx, cy, sk = [float(v) for v in row[:5]]
    return Camera(intrinsics=[[fx, sk, cx], [0, fy, cy], [0, 0, 1]], translation=row[14:17].astype(np.float64),
                  rotation=row[5:14].astype(np.float64).reshape(3, 3))


def test_device_sampler_matches_the_restatement_on_config4_at_2048_envs():
    """(a) 2048 envs, a 64-env slice: status, chosen pixel pair and depth equal the restatement on the oracle's
    render of the same envs; the 4-DoF action is Grasp2D.from_vector(...).as_4dof() with the env's noisy camera."""
    from robovat_amd import lib
    from robovat_amd.envs.grasp.grasp_2d import Grasp2D
    from oracle import orc
    env_cfg = configs.grasp_env_config(**NOISE)
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    seed, m = 21, 3
    world = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=2048, seed=seed, shape_names=names), scene, device=0)
    ref = orc.OracleWorld(configs.make_rv_config(env_cfg=env_cfg, n_envs=64, seed=seed, shape_names=names), scene, double=False)
    world.reset(); ref.reset()
    g, a4, st = world.policy_antipodal(lib.antipodal_params(), m)
    g, a4, st = g.cpu().numpy()[:64], a4.cpu().numpy()[:64], st.cpu().numpy()[:64]
    cam = world.camera().cpu().numpy()[:64]
    assert np.array_equal(cam, ref.camera().astype(np.float32))
    assert np.ptp(cam[:, 0]) > 0.5            # the per-env calibration matters
    rnd = world.policy_random(m).cpu().numpy()[:64, 0]
    P = _policy_params()
    flagged, found = [], 0
    for i in range(64):
        depth, _ = ref.render(i)
        h = host.sample(depth, P, cam[i, 0], cam[i, 2], seed=seed, gid=i, macro_index=m)
        if h['status'] != st[i] or (h['status'] == 1 and not np.array_equal(h['grasp'][:4], g[i, :4])):
            assert h.get('borderline_before_choice', False), (i, h['status'], st[i], h.get('grasp'), g[i])
            flagged.append(i)
            continue
        camera = _camera(cam[i])
        if st[i] == 1:
            found += 1
            assert abs(g[i, 4] - h['grasp'][4]) <= 1e-6 * abs(h['grasp'][4])
            want = np.array(Grasp2D.from_vector(g[i], camera=camera).as_4dof())
            assert np.allclose(a4[i, :3], want[:3], atol=1e-4), (i, a4[i], want)
            assert abs(np.angle(np.exp(1j * (a4[i, 3] - want[3])))) < 1e-4
        else:
            assert np.array_equal(a4[i], rnd[i])
            back = np.array(Grasp2D.from_vector(g[i], camera=camera).as_4dof())
            assert np.allclose(back[:3], rnd[i, :3], atol=1e-4)
    print('antipodal vs restatement: %d / 64 grasps, borderline envs %s' % (found, flagged))
    assert len(flagged) <= 4
    assert found >= 40
    world.close()


def _golden():
    with open(os.path.join(HERE, 'golden', 'antipodal_golden.json')) as f:
        return json.load(f)['cases']


def _bits(s, e):
    raw = np.frombuffer(zlib.decompress(base64.b64decode(s)), np.uint8)
    return np.unpackbits(raw)[:e * e].reshape(e, e).astype(bool)


def test_device_sampler_on_the_reference_golden_images():
    """(b) the golden images through d_depth: the chosen pair is in the reference's passing set; statuses agree."""
    from robovat_amd import lib
    n = 8
    for case in _golden():
        img = host.synth_image(case['spec'])
        h_, w_ = img.shape
        K = np.array(case['intrinsics'])
        env_cfg = configs.grasp_env_config(**{'KINECT2.DEPTH.HEIGHT': h_, 'KINECT2.DEPTH.WIDTH': w_,
                                              'KINECT2.DEPTH.INTRINSICS': K.tolist()})
        scene, names = scenes.make_scene(env_cfg=env_cfg)
        world = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=4, shape_names=names), scene, device=0)
        world.reset()
        p = case['params']
        cfg = {'SAMPLER': {k: v for k, v in p.items() if k != 'GRIPPER_WIDTH'}, 'GRIPPER_WIDTH': p['GRIPPER_WIDTH']}
        g, _, st = world.policy_antipodal(lib.antipodal_params(cfg), 0, depth=np.broadcast_to(img, (n, h_, w_)).copy())
        g, st = g.cpu().numpy(), st.cpu().numpy()
        edges = [tuple(e) for e in case['edges']]
        r0, c0 = (p['CROP'] or [0, 0])[:2]
        passing = _bits(case['passing_bits'], len(edges)) if edges else None
        index = {e: k for k, e in enumerate(edges)}
        for i in range(n):
            h = host.sample(img, p, K[0, 0], K[0, 2], seed=4, gid=i, macro_index=0)
            assert st[i] == h['status'], (case['name'], i, st[i], h['status'])
            if st[i] == 1:
                a = index[(int(g[i, 1]) - r0, int(g[i, 0]) - c0)]
                b = index[(int(g[i, 3]) - r0, int(g[i, 2]) - c0)]
                assert passing[a, b], (case['name'], i)
        if not edges:
            assert (st == 0).all()
        if all(s['error'] for s in case['samples']):
            assert (st <= -1).all(), case['name']
        if all(s['grasp'] for s in case['samples']) and p['MAX_REJECTION_SAMPLES'] >= case['n_valid']:
            assert (st == 1).all(), case['name']
        world.close()


def test_policy_end_to_end_in_both_action_types_and_single_env():
    """(c) VecGrasp4DofEnv(2048) CUBOID and IMAGE, Grasp4DofEnv: several steps; failed rows carry the random draw;
    the same seed reproduces the same actions."""
    from robovat_amd import envs, policies
    for action_type in ('CUBOID', 'IMAGE'):
        cfg = configs.grasp_env_config(**{'ACTION.TYPE': action_type})
        runs = []
        for _ in range(2):
            env = envs.VecGrasp4DofEnv(2048, config=cfg, seed=9)
            policy = policies.AntipodalGrasp4DofPolicy(env)
            obs = env.reset()
            acts = []
            for step in range(3):
                a = policy.action(obs)
                assert tuple(a.shape) == (2048, 4 if action_type == 'CUBOID' else 5)
                st = env.antipodal_status.cpu().numpy()
                assert set(np.unique(st)) <= {1, 0, -1, -2, -3} and (st == 1).mean() > 0.5
                if action_type == 'CUBOID':
                    rnd = env.world.policy_random(env._macro_index).cpu().numpy()[:, 0]
                    assert np.array_equal(a.cpu().numpy()[st != 1], rnd[st != 1])
                acts.append(a.cpu().numpy())
                obs, reward, done, _ = env.step(a)
                print('%s step %d: status %s, success rate %.3f' % (action_type, step, {int(k): int((st == k).sum()) for k in np.unique(st)},
                                                                    float(reward.float().mean())))
                obs = env.reset()
            runs.append(np.stack(acts))
            env.close()
        assert np.array_equal(runs[0], runs[1])
    env = envs.Grasp4DofEnv(seed=3)
    policy = policies.AntipodalGrasp4DofPolicy(env)
    ok = 0
    for _ in range(4):
        obs = env.reset()
        try:
            a = policy.action(obs)
        except ValueError:
            continue
        assert a.shape == (4,)
        env.step(a)
        ok += 1
    assert ok >= 1
    env.close()


def test_invalid_parameters_raise_value_error():
    """(d) the library's checks, through rv_last_error."""
    import copy
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
            world.policy_antipodal(lib.antipodal_params(cfg), 0)
        assert 'rv_policy_antipodal' in str(e.value), key
    world.close()
    push_scene, push_names = scenes.make_scene()
    push = lib.World(configs.make_rv_config(n_envs=2, shape_names=push_names), push_scene, device=0)
    with pytest.raises(ValueError):
        push.policy_antipodal(lib.antipodal_params(), 0)
    push.close()
