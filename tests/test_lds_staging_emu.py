"""CPU: the lane phases of rv_dev_env.h that load everything they read before their first store (DESIGN.md §10,
"LDS staging") are compiled by the lane emulator from the same source.  A value forwarded from the wrong place, a load
moved over its producer or an index clamped wrongly changes a bit of the state, so the emulator must still equal the
float oracle bit for bit (`_check` of test_emu_parity: body, joint and link states, env counters, manifold sizes)."""
import ctypes as C

from robovat_amd import configs, scenes
from test_emu_parity import Emu, _check, emu  # noqa: F401  (the lane emulator's fixture and getters)

CONCAVE = dict(TASK_NAME='crossing', LAYOUT_ID=0, MOVABLE_NAME='CONCAVE')


def _pair(emu, n, seed, **over):  # noqa: F811
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(**over), n_envs=n, seed=seed, shape_names=names)
    ref = orc.OracleWorld(cfg, scene, double=False)
    e = Emu(emu, cfg, scene)
    ref.reset(); emu.emu_reset(e.h, None)
    _check(e, ref)
    return e, ref


def _steps(emu, e, ref, k):  # noqa: F811
    for i in range(k):
        a = ref.policy_random(i)
        ref.set_actions(a); emu.emu_set_actions(e.h, a.ctypes.data_as(C.c_void_p))
        ref.step_macro(); emu.emu_step_macro(e.h)
        _check(e, ref)


def test_config2_scene_two_steps(emu):  # noqa: F811
    """Config-2 scene, 2 envs x 2 env.step(), seed 5: motor / FK / collider phases in every substep, arm-body owners
    through the owner / gate phase, coast segments with their clearances, wake-ups through the body-velocity phase."""
    e, ref = _pair(emu, 2, 5)
    _steps(emu, e, ref, 2)


def test_concave_bodies_fill_the_vertex_phases(emu):  # noqa: F811
    """'crossing' / CONCAVE, 2 envs x 1 step, seed 17: several hulls per body, so a lane of the vertex phases holds a
    vertex of more than one body and lanes beyond 15 hold vertices at all (more than 64 items per phase)."""
    e, ref = _pair(emu, 2, 17, MAX_STEPS=3, **CONCAVE)
    _steps(emu, e, ref, 1)


def test_a_launch_that_begins_with_a_reset(emu):  # noqa: F811
    """Episodes of one step under auto-reset: the second one-step rollout begins with reset + settle -- substeps without an
    arm, on scratch the previous episode left behind -- and goes straight on to a step."""
    e, ref = _pair(emu, 2, 5, MAX_STEPS=1)
    for k in range(2):
        ref.rollout(1, k, True); emu.emu_rollout(e.h, 1, k, 1)
        _check(e, ref)
    assert (ref.env_counters()[:, 2] >= 1).all()      # (every env finished an episode, so the second launch reset it)
