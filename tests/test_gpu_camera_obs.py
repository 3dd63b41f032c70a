"""The device's camera products beyond their defaults (MI355X): k_render against the independent float64 ray caster of
tests/camera_host.py, and k_point_cloud -- bit for bit against the float oracle and against the contract of
group_by_labels / downsample on the device's own render -- for every num_points, crop box and view of
camera_host.CLOUD_CASES, observed directly and through a recorded rollout.

The observation kernels are compiled once, in rv_kernels.hip; the two env-kernel builds (RV_ENV_OCC) differ in the env
kernel only and fill the same ObsSnap, so the tests run on the default build."""
import ctypes as C

import numpy as np
import pytest

from robovat_amd import abi

import camera_host as ch
from test_camera_host import cloud_cfg, compare_renders, render_case

pytestmark = pytest.mark.gpu


def _worlds(cfg, scene):
    from robovat_amd import lib
    from oracle import orc
    w, ref = lib.World(cfg, scene, device=0), orc.OracleWorld(cfg, scene, double=False)
    w.reset(); ref.reset()
    return w, ref


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('name', ['push', 'concave'])
def test_render_vs_independent_ray_cast(name):
    """World.render() == ray cast from hull vertices, table planes and link boxes in float64, from the device's own
    body states, link frames and calibrations: the assertions and bounds of
    test_camera_host.test_oracle_render_vs_independent_ray_cast."""
    from robovat_amd import lib
    cfg, scene, bound = render_case(name)
    w = lib.World(cfg, scene, device=0)
    w.reset()
    depth, seg = w.render()
    compare_renders(cfg, scene, bound, _np(w.body_state()), _np(w.body_params()), _np(w.link_poses()), _np(w.camera()),
                    _np(depth), _np(seg))
    w.close()


_FIRST_LOOKS = {}


def device_first_look(cfg):
    """Segmentation masks and body states after reset of a device world with cfg's view (one world per view)."""
    from robovat_amd import lib
    key = tuple(cfg.cam_translation)
    if key not in _FIRST_LOOKS:
        w = lib.World(cfg, cloud_cfg()[1], device=0)
        w.reset()
        _FIRST_LOOKS[key] = _np(w.render()[1]), _np(w.body_state())
        w.close()
    return _FIRST_LOOKS[key]


@pytest.mark.parametrize('name,spec,need', ch.CLOUD_CASES, ids=[c[0] for c in ch.CLOUD_CASES])
def test_point_cloud_beyond_the_defaults(name, spec, need):
    """World.observe(point_cloud=True) == OracleWorld.point_cloud() bit for bit, and the cloud keeps the contract of
    camera_host.check_cloud against the device's own render, reaching the cases the parameter set is there for."""
    cfg, scene = cloud_cfg()
    ch.apply_cloud_case(cfg, spec, device_first_look)
    w, ref = _worlds(cfg, scene)
    got = _np(w.observe(point_cloud=True)['point_cloud'])
    want = ref.point_cloud()
    assert got.shape == want.shape == (6, abi.RV_MAXB, int(cfg.num_points), 3)
    assert np.array_equal(got, want), np.abs(got - want).max()
    depth, seg = w.render()
    kinds = ch.check_clouds(cfg, got, _np(depth), _np(seg), _np(w.camera()))
    print(name, int(cfg.num_points), kinds)
    assert all(kinds.get(k, 0) > 0 for k in need), (need, kinds)
    w.close()


@pytest.mark.parametrize('name', ['crop', 'P1000_dz-0.7'])
def test_recorded_point_cloud_beyond_the_defaults(name):
    """rollout_record(2, point_cloud=True) renders its clouds afterwards, from the ObsSnap rows taken at observation
    time: both recorded rows equal the oracle's cloud after the same step bit for bit, and the last row keeps the
    contract against the device's render of the state the rollout ends in."""
    spec, need = [(s, n) for c, s, n in ch.CLOUD_CASES if c == name][0]
    cfg, scene = cloud_cfg()
    ch.apply_cloud_case(cfg, spec, device_first_look)
    w, ref = _worlds(cfg, scene)
    obs, _, _ = w.rollout_record(2, first_macro_index=0, auto_reset=True, point_cloud=True)
    rows = _np(obs['point_cloud'])
    for k in range(2):
        ref.rollout(1, k, True)
        want = ref.point_cloud()
        assert np.array_equal(rows[k], want), (k, np.abs(rows[k] - want).max())
    assert np.array_equal(_np(w.body_state()), ref.body_state().astype(np.float32))
    depth, seg = w.render()
    kinds = ch.check_clouds(cfg, rows[1], _np(depth), _np(seg), _np(w.camera()))
    print(name, int(cfg.num_points), kinds)
    assert all(kinds.get(k, 0) > 0 for k in need), (need, kinds)
    w.close()


@pytest.mark.parametrize('P', [0, abi.RV_PC_MAXPIX + 1])
def test_observe_rejects_num_points_outside_the_buffer(P):
    """rv_observe with a point-cloud buffer and num_points outside [1, RV_PC_MAXPIX]: RV_ERR_VALUE, no launch."""
    import torch
    from robovat_amd import lib
    cfg, scene = cloud_cfg()
    cfg.num_points = P
    w = lib.World(cfg, scene, device=0)
    w.reset()
    out, b = w._obs_buffers((w.n,), True, False)
    room = torch.zeros((w.n, abi.RV_MAXB, max(P, 1), 3), dtype=torch.float32, device=w.device)
    b.d_point_cloud = room.data_ptr()
    assert w.lib.rv_observe(w.h, C.byref(b)) == abi.RV_ERR_VALUE
    with pytest.raises(ValueError):
        lib.check(w.lib.rv_observe(w.h, C.byref(b)))
    assert not _np(room).any()
    w.close()
