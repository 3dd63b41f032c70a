"""The float oracle's camera products against tests/camera_host.py (CPU): its depth image and segmentation mask against
an independent float64 ray caster, and its point cloud against the contract of group_by_labels / downsample beyond the
default num_points / crop / view.  tests/test_gpu_camera_obs.py asks the same of the device."""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes

import camera_host as ch
from test_camera_noise import NOISE
from test_static_body import WALLS

CONCAVE = dict(TASK_NAME='crossing', LAYOUT_ID=0, MOVABLE_NAME='CONCAVE', MIN_MOVABLE_BODIES=2)
# name -> (env config, seed, depth bound).  Seed 4 throughout, except behind the wall: it hides a body of one env at
# seed 4, and every active body has to be in the image for the comparison to mean something
RENDER_CASES = {
    'push': (lambda: configs.push_env_config(), 4, 'convex'),
    'concave': (lambda: configs.push_env_config(**CONCAVE), 4, 'concave'),
    'grasp': (lambda: configs.grasp_env_config(), 4, 'convex'),
    'camera_noise': (lambda: configs.push_env_config(**NOISE), 4, 'convex'),
    'wall': (lambda: configs.push_env_config(**WALLS[1]), 3, 'convex'),
}
# largest |float render - float64 ray cast| over the agreeing pixels of the ten images below, in metres of eye depth:
# 1.9e-6 with convex templates (push 1.9e-6, grasp 3.1e-7, camera noise 1.2e-6, wall 1.3e-6) and 1.2e-5 with concave
# ones (the float32 plane tables of the decomposed templates against their own vertices; the double oracle shows the
# same gap).  The bounds are 4 x that: float32 rounding through the ten-odd operations of a ray / plane intersection
# at ~1 m varies by a small factor with the pose
DEPTH_BOUND = {'convex': 4 * 1.9e-6, 'concave': 4 * 1.2e-5}


def render_case(name, n=2):
    make, seed, kind = RENDER_CASES[name]
    env_cfg = make()
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, shape_names=names), scene, DEPTH_BOUND[kind]


def compare_renders(cfg, scene, bound, state, params, links, cams, depth, seg):
    """Every env's image (depth / seg [n, H, W]) against the ray cast of that env's state; prints what it measured."""
    for i in range(len(depth)):
        ref = ch.raycast(cfg, scene, state[i], params[i], links[i], ch.camera_of(cfg, cams[i]))
        present = [b for b in range(abi.RV_MAXB) if params[i][b][0]] + [abi.RV_MAXB, abi.RV_MAXB + 1]
        err, share = ch.compare_render(depth[i], seg[i], ref, present)
        print('env %d: max |depth - ray cast| %.3e m, undecided pixels %.3f %%' % (i, err, 100 * share))
        assert err <= bound, (err, bound)


@pytest.mark.parametrize('name', list(RENDER_CASES))
def test_oracle_render_vs_independent_ray_cast(name):
    """orc_render (float) == ray cast from hull vertices, table planes and link boxes in float64: the same label on
    every pixel the ray caster decides (at most 0.2 % per image are undecided: within EPS = 1e-4 m of a silhouette or a
    depth tie), the arm, the table and every active body among the compared pixels, and the depth of agreeing pixels
    within DEPTH_BOUND (measured above: 1.9e-6 m convex, 1.2e-5 m concave; bounds 7.6e-6 and 4.8e-5 m)."""
    from oracle import orc
    cfg, scene, bound = render_case(name)
    w = orc.OracleWorld(cfg, scene, double=False)
    w.reset()
    images = [w.render(i) for i in range(w.n)]
    compare_renders(cfg, scene, bound, w.body_state(), w.body_params(), w.link_poses(), w.camera(),
                    [d for d, _ in images], [s for _, s in images])


def cloud_cfg(n=6, seed=4):
    scene, names = scenes.make_scene()
    return configs.make_rv_config(env_cfg=configs.push_env_config(), n_envs=n, seed=seed, shape_names=names), scene


_FIRST_LOOKS = {}


def oracle_first_look(cfg):
    """Segmentation masks and body states after reset of an oracle world with cfg's view (one world per view)."""
    from oracle import orc
    key = tuple(cfg.cam_translation)
    if key not in _FIRST_LOOKS:
        w = orc.OracleWorld(cfg, scenes.make_scene()[0], double=False)
        w.reset()
        _FIRST_LOOKS[key] = np.stack([w.render(i)[1] for i in range(w.n)]), w.body_state()
    return _FIRST_LOOKS[key]


@pytest.mark.parametrize('name,spec,need', ch.CLOUD_CASES, ids=[c[0] for c in ch.CLOUD_CASES])
def test_oracle_point_cloud_beyond_the_defaults(name, spec, need):
    """orc_point_cloud keeps the contract of group_by_labels / downsample (camera_host.check_cloud; members from the
    oracle's own full render) for every num_points, crop box and view of camera_host.CLOUD_CASES, and each set reaches
    the cases it is there for."""
    from oracle import orc
    cfg, scene = cloud_cfg()
    ch.apply_cloud_case(cfg, spec, oracle_first_look)
    w = orc.OracleWorld(cfg, scene, double=False)
    w.reset()
    images = [w.render(i) for i in range(w.n)]
    kinds = ch.check_clouds(cfg, w.point_cloud(), [d for d, _ in images], [s for _, s in images], w.camera())
    print(name, int(cfg.num_points), kinds)
    assert all(kinds.get(k, 0) > 0 for k in need), (need, kinds)
