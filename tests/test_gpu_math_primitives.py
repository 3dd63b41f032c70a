"""The scalar primitives of robovat_amd/csrc/rv_dev_math.h on the MI355X (tests/probe/rv_math_probe.hip, compiled for
gfx950 with exactly the product's flags by __graft_entry__.build()).

* Bit parity: the device equals the host compile of the same header, word for word, over the shared inputs of
  tests/probe/inputs.py -- the inputs on which tests/test_math_primitives.py holds the host compile to the float
  oracle and to float64.  This is where the claims behind all bit parity are tested away from scene values:
  correctly rounded sqrt and division, denormals kept, v_med3_f32 == fclampr, rint ties to even, (int)k.
* Philox known answers on the device.
* End to end: body quaternions of the gimbal-lock family go through the product's observation write and come out as
  the oracle's bits and within the rotation-error bound.

A missing or stale device probe is an error (probe_build.DeviceProbe raises), never a skip.
"""
import numpy as np
import pytest

from probe import build as probe_build, inputs
from robovat_amd import abi, configs, scenes
from test_math_primitives import euler_bound, euler_round_trip_error, first_difference

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope='module')
def device():
    return probe_build.DeviceProbe()


@pytest.fixture(scope='module')
def host():
    return probe_build.host_probe()


@pytest.mark.parametrize('name', sorted(probe_build.FUNCS))
def test_device_equals_host_compile_bit_for_bit(device, host, name):
    """One launch over the whole input array of the function; uint32 views, so -0 is not +0."""
    ins, k = inputs.cases()[name]
    want = host.call(name, *ins, k=k)
    got = device.call(name, *ins, k=k)
    assert got.dtype == want.dtype and got.shape == want.shape
    msg = first_difference(name, ins, got, want)
    assert msg is None, msg


def test_fclamp_pm_is_fclampr_on_the_device(device):
    """v_med3_f32(x, -b, b) == the two compare-select pairs, on the device itself, for every non-NaN x and b > 0."""
    (x, b), _ = inputs.cases()['p_fclamp_pm']
    msg = first_difference('fclamp_pm vs fclampr', (x, b), device.call('p_fclamp_pm', x, b), device.call('p_fclampr_pm', x, b))
    assert msg is None, msg


def test_philox_known_answers_on_the_device(device):
    ctr = np.array([k[0] for k in inputs.PHILOX_KAT], np.uint32)
    key = np.array([k[1] for k in inputs.PHILOX_KAT], np.uint32)
    got = device.call('p_philox', ctr, key)
    for j, (_, _, out) in enumerate(inputs.PHILOX_KAT):
        assert tuple(int(v) for v in got[j]) == out, (j, [hex(int(v)) for v in got[j]])


def test_gimbal_lock_poses_through_the_observation():
    """64 PushEnv worlds of the default scene, device and float oracle; after reset every body is given a quaternion
    of the gimbal-lock family (positions stay, velocities zero) and the observation is taken with NO step.  The Euler
    angles of `pose`, the yaw of `pose2d` and `yaw_cossin` are the oracle's bits, rebuild the rotation that was set
    within the bound of tests/test_math_primitives.py, and (cos, sin) is within 2^-22 of the returned yaw's."""
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(), n_envs=64, seed=31, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    ref = orc.OracleWorld(cfg, scene, double=False)
    world.reset(); ref.reset()
    st = ref.body_state().astype(F)
    assert np.array_equal(world.body_state().cpu().numpy(), st)
    e, q = inputs.gimbal_family()
    # evenly through the family (one block per half-decade of d = pi/2 - |pitch| from 1e-9 to 1, d = 0 last): some of
    # every half-decade and of the exact lock, both signs of pitch
    pick = np.linspace(0, q.shape[0] - 1, 64 * abi.RV_MAXB).astype(np.int64)
    pick[-8:] = np.arange(q.shape[0] - 8, q.shape[0])
    qs = q[pick].reshape(64, abi.RV_MAXB, 4)
    st[..., 3:7] = qs
    st[..., 7:] = 0
    world.set_body_state(st); ref.set_body_state(st)
    assert np.array_equal(world.body_state().cpu().numpy()[..., 3:7].view(np.uint32), qs.view(np.uint32))
    got = {k: v.cpu().numpy() for k, v in world.observe(pose_modes=True).items()}
    want = ref.observe(full=True)
    on = got['body_mask'] > 0
    assert np.array_equal(got['body_mask'], want['body_mask'].astype(F)) and on.sum() >= 64 * 2
    for key in ('pose', 'pose2d', 'yaw_cossin'):
        assert np.array_equal(got[key].view(np.uint32), want[key].astype(F).view(np.uint32)), key
    eu = got['pose'][..., 3:6][on]
    assert np.array_equal(got['pose2d'][..., 2][on].view(np.uint32), np.ascontiguousarray(eu[:, 2]).view(np.uint32))
    err = euler_round_trip_error(qs[on], eu)
    cy = inputs.cos_pitch(qs[on])
    assert (cy < 3e-4).sum() >= 16 and (cy > 1e-2).sum() >= 16
    ratio = err / euler_bound(cy)
    i = int(ratio.argmax())
    print('observation: worst rotation error / bound = %.3f (%.3e rad at cy = %.3e)' % (ratio[i], err[i], cy[i]))
    assert ratio[i] <= 1.0, 'rotation error %.3e rad at cy = %.3e: %.1f x the bound' % (err[i], cy[i], ratio[i])
    yaw = eu[:, 2].astype(np.float64)
    cs = got['yaw_cossin'][on].astype(np.float64)
    dev = np.abs(cs - np.stack([np.cos(yaw), np.sin(yaw)], 1)).max()
    assert dev <= 2.0 ** -22, dev
    world.close()
