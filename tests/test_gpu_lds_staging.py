"""GPU: the env kernel with its lane phases staged (every load of a phase ahead of its first store: DESIGN.md §10, "LDS
staging") still computes what the float oracle computes, on both code objects.

Tolerances: the staging moves loads and stores and changes no floating-point instruction, and the kernels match the float
oracle operation for operation: body and joint states agree to 1e-6 and every integer (env counters, manifold sizes,
substeps) is equal -- the bounds of tests/test_gpu_narrow_phase_pairs.py.
"""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes

CONCAVE = dict(TASK_NAME='crossing', LAYOUT_ID=0, MOVABLE_NAME='CONCAVE')


def _cfg(n, seed, **over):
    scene, names = scenes.make_scene()
    return configs.make_rv_config(env_cfg=configs.push_env_config(**over), n_envs=n, seed=seed, shape_names=names), scene


def _world(n, seed, **over):
    from robovat_amd import lib
    cfg, scene = _cfg(n, seed, **over)
    return lib.World(cfg, scene, device=0)


def _oracle(n, seed, **over):
    from oracle import orc
    cfg, scene = _cfg(n, seed, **over)
    return orc.OracleWorld(cfg, scene, double=False)


def _cmp(world, ref, tol=1e-6, lo=0):
    """`ref` holds the envs lo .. lo + ref.n of `world`."""
    n = ref.body_state().shape[0]
    err = np.abs(world.body_state().cpu().numpy()[lo:lo + n] - ref.body_state().astype(np.float32)).max()
    assert err <= tol, err
    jerr = np.abs(world.joint_state().cpu().numpy()[lo:lo + n] - ref.joint_state().astype(np.float32)).max()
    assert jerr <= tol, jerr
    assert np.array_equal(world.env_counters().cpu().numpy()[lo:lo + n], ref.env_counters())
    assert np.array_equal(world.manifold_counts().cpu().numpy()[lo:lo + n], ref.manifold_counts())


@pytest.fixture(scope='module')
def rollout_ref():
    """Config-2 scene, 16 envs, seed 5, after a 3-step rollout with auto-reset: computed once, read only."""
    ref = _oracle(16, 5)
    ref.reset(); ref.rollout(3, 0, True)
    return ref


@pytest.mark.gpu
def test_recorded_rollout_on_the_register_rich_build(rollout_ref):
    world = _world(16, 5)
    assert world.env_kernel_build() == abi.RV_ENV_BUILD_OCC1
    world.reset()
    world.rollout_record(3, auto_reset=True)
    _cmp(world, rollout_ref)
    assert world.stats()['substeps'] == rollout_ref.stats()['substeps']
    world.close()


@pytest.mark.gpu
def test_recorded_rollout_on_the_two_waves_per_simd_build(rollout_ref):
    """The same world with one env more than the GPU has SIMDs: launched as the 256-register code object, where the
    staged phases have the fewest registers to stage into.  First and last 16 envs against oracle slices."""
    import torch
    n = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    world = _world(n, 5)
    assert world.env_kernel_build() == 2
    world.reset()
    world.rollout_record(3, auto_reset=True, point_cloud=False)
    _cmp(world, rollout_ref)
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(), n_envs=16, seed=5, env_id_offset=n - 16, shape_names=names)
    tail = orc.OracleWorld(cfg, scene, double=False)
    tail.reset(); tail.rollout(3, 0, True)
    _cmp(world, tail, lo=n - 16)
    world.close()


@pytest.mark.gpu
def test_concave_bodies_two_steps():
    """8 envs x 2 steps, CONCAVE, seed 21: every lane of the vertex phases holds hull vertices of several bodies."""
    world, ref = _world(8, 21, **CONCAVE), _oracle(8, 21, **CONCAVE)
    world.reset(); ref.reset()
    _cmp(world, ref)
    for k in range(2):
        a = ref.policy_random(k)
        world.set_actions(a); ref.set_actions(a)
        world.step_macro(); ref.step_macro()
        _cmp(world, ref)
        assert world.stats()['substeps'] == ref.stats()['substeps']
    world.close()
