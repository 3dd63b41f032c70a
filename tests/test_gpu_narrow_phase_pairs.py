"""The narrow phase deals its convex queries to the four 16-lane groups by PAIR (rv_dev_env.h: collide_query /
collide_apply): the pairs of one manifold are queried side by side, round by round, and their results enter the
manifold afterwards in pair order.  What the float oracle pins -- the order of man_add within a manifold, the `age`
decision of every pair, the simplex cache each query starts from and the one the pass leaves, the pair totals -- must
come out as when one group works through an owner's pairs one after the other.

Tolerances: the kernels match the float oracle operation for operation, so body and joint states agree to 1e-6 and
every integer (env counters with pairs_last, manifold sizes, substeps) is equal.
"""
import ctypes as C

import numpy as np
import pytest

from robovat_amd import configs, scenes
from test_emu_parity import Emu, _check, emu  # noqa: F401  (the lane emulator's fixture and getters)

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
    assert np.array_equal(world.env_counters().cpu().numpy()[lo:lo + n], ref.env_counters())      # (pairs_last among them)
    assert np.array_equal(world.manifold_counts().cpu().numpy()[lo:lo + n], ref.manifold_counts())


@pytest.fixture(scope='module')
def rollout_ref():
    """Case 1's world (config-2 scene, 16 envs, seed 5) after a 3-step rollout with auto-reset: computed once, read only."""
    ref = _oracle(16, 5)
    ref.reset(); ref.rollout(3, 0, True)
    return ref


@pytest.mark.gpu
def test_config2_scene_arm_body_owners_with_several_near_boxes():
    """Arm-body owners with several near collider boxes beside table and body-body owners: items of several manifolds
    share a round."""
    world, ref = _world(16, 5), _oracle(16, 5)
    world.reset(); ref.reset()
    _cmp(world, ref)
    for k in range(3):
        a = ref.policy_random(k)
        world.set_actions(a); ref.set_actions(a)
        world.step_macro(); ref.step_macro()
        _cmp(world, ref)
        assert world.stats()['substeps'] == ref.stats()['substeps']
    world.close()


@pytest.mark.gpu
def test_concave_owners_with_more_pairs_than_a_round_holds():
    """Concave bodies: up to 16 pairs per owner -- several rounds and several pairs per manifold, the smallest shape where
    the apply order and the hand-over of the simplex cache can go wrong."""
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


@pytest.mark.gpu
def test_recorded_rollout_on_the_register_rich_build(rollout_ref):
    world = _world(16, 5)
    world.reset()
    world.rollout_record(3, auto_reset=True)
    _cmp(world, rollout_ref)
    assert world.stats()['substeps'] == rollout_ref.stats()['substeps']
    world.close()


@pytest.mark.gpu
def test_recorded_rollout_on_the_two_waves_per_simd_build(rollout_ref):
    """One env more than the GPU has SIMDs: the smallest world that is launched as k_env_occ2 (the 256-register code
    object).  Its first 16 envs are case 1's, its last 16 are checked against an oracle slice of their own."""
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


def test_emulated_flat_pair_list_with_more_than_four_pairs_per_owner(emu):  # noqa: F811
    """CPU: the lane emulator shares the query stage's source (one lane per group works): the 'crossing' / CONCAVE scene,
    2 envs x 1 step, equals the float oracle bit for bit -- the flat item list with owners of more than four pairs."""
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(MAX_STEPS=3, **CONCAVE), n_envs=2, seed=17, shape_names=names)
    ref = orc.OracleWorld(cfg, scene, double=False)
    e = Emu(emu, cfg, scene)
    ref.reset(); emu.emu_reset(e.h, None)
    _check(e, ref)
    a = ref.policy_random(0)
    ref.set_actions(a); emu.emu_set_actions(e.h, a.ctypes.data_as(C.c_void_p))
    ref.step_macro(); emu.emu_step_macro(e.h)
    _check(e, ref)
