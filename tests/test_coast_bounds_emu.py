"""The body clearance of coasting (coast_measure_clearances in robovat_amd/csrc/rv_dev_env.h) on the CPU.

A coasting run skips the wake test of every (sleeping body, collider box) pair for as long as the box's travel bound
stays below an admissible travel measured on the last fresh kinematics: the largest of `largest axis gap - R`,
`(AABB distance - R) / sqrt 3` and the distance bound of the last wake query (R = wake range + 2 margin).  The float
oracle never coasts -- it runs every test in every substep -- so "the emulated kernel equals the oracle bit for bit"
says that every skipped test would have said no.

(a) four scenes, emulator against oracle; (b) the event counters of the emulator built with -DRV_EMU_COUNT (as
tools/emu_counts.py builds it): the scenes are what they claim, the work is unchanged and the run boundaries are
fewer; (c) the inequality behind the bound, restated in numpy.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from robovat_amd import abi, configs, scenes
from test_emu_parity import EMU_DIR, Emu, emu_library

# ---------------------------------------------------------------------------------------------------------------------
# the four scenes (tests/test_gpu_coast_bounds.py runs the same four on the GPU)

SCENES = ('default_push', 'four_bodies', 'diagonal_sleeper', 'grasp')
DIAGONAL_OFFSET = 0.09          # metres, along each of x and y


def make_case(name, n, seed):
    """(cfg, scene) of one of the four scenes."""
    if name == 'grasp':
        env_cfg = configs.grasp_env_config()
        scene, names = scenes.make_scene(env_cfg=env_cfg)
    else:
        over = dict(MIN_MOVABLE_BODIES=4, MAX_MOVABLE_BODIES=4) if name == 'four_bodies' else {}
        env_cfg = configs.push_env_config(**over)
        scene, names = scenes.make_scene()
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, shape_names=names), scene


def diagonal_state(ref, cfg):
    """The body state of the 'diagonal_sleeper' scene, from the oracle after its reset: body 0 of every env is moved
    to DIAGONAL_OFFSET along x AND y from the point above which the first push starts, on the side the push moves away
    from.  The fingers come down beside it and leave: while they do, the body is off the fingers in x, in y and in z
    at once.  (Whoever applies the state lets the bodies come to rest -- wait_until_stable -- before the first step:
    rv_set_body_state wakes them.)"""
    from oracle import orc
    a = ref.policy_random(0)
    st = ref.body_state().astype(np.float32)
    for i in range(cfg.n_envs):
        s, e = orc.eval_waypoints(cfg, a[i, 0])
        side = np.sign(s[:2] - e[:2])
        side[side == 0] = 1
        st[i, 0, 0:2] = s[:2] + side * DIAGONAL_OFFSET
        st[i, 0, 7:] = 0
    return st


def _oracle(cfg, scene):
    from oracle import orc
    return orc.OracleWorld(cfg, scene, double=False)


def run_oracle(name, n, seed, steps):
    """The oracle's side of a scene: reset, (the diagonal scene's state), `steps` env steps in one rollout.  Returns the
    oracle world and the state that was set (None where the scene sets none)."""
    cfg, scene = make_case(name, n, seed)
    ref = _oracle(cfg, scene)
    ref.reset()
    st = None
    if name == 'diagonal_sleeper':
        st = diagonal_state(ref, cfg)
        ref.set_body_state(st); ref.wait_until_stable()
    ref.rollout(steps, 0, True)
    return ref, st


def run_emu(lib, name, n, seed, steps, st):
    cfg, scene = make_case(name, n, seed)
    e = Emu(lib, cfg, scene)
    lib.emu_reset(e.h, None)
    if st is not None:
        lib.emu_set_body_state(e.h, np.ascontiguousarray(st, np.float32).ctypes.data_as(C.c_void_p))
        lib.emu_wait_until_stable(e.h, C.c_float(0.005), C.c_float(0.005), 100, 100, 2000)
    lib.emu_rollout(e.h, steps, 0, 1)
    return e


# ---------------------------------------------------------------------------------------------------------------------
# (a) emulator == float oracle, bit for bit

N_A, STEPS_A, SEED_A = 8, 3, 4


@pytest.fixture(scope='module')
def emu():
    return emu_library('inline')


@pytest.mark.parametrize('name', SCENES)
def test_emulated_kernel_equals_the_float_oracle(emu, name):
    """8 envs x 3 steps: body states, joint states, env counters and manifold counts."""
    ref, st = run_oracle(name, N_A, SEED_A, STEPS_A)
    e = run_emu(emu, name, N_A, SEED_A, STEPS_A, st)
    assert np.array_equal(e.body_state(), ref.body_state().astype(np.float32))
    assert np.array_equal(e.joint_state(), ref.joint_state().astype(np.float32))
    assert np.array_equal(e.counters(), ref.env_counters())
    assert np.array_equal(e.manifolds(), ref.manifold_counts())
    assert ref.stats()['env_steps'] == N_A * STEPS_A


# ---------------------------------------------------------------------------------------------------------------------
# (b) the counters

# tools/emu_counts.py 16 4 on the commit before the bound was tightened (seed 1234; the emulator is deterministic)
PARENT_RUNS, PARENT_REMEASURED = 11063, 8763
SUBSTEPS, HEAVY, IK_CALLS = 343900, 5837, 1087


@pytest.fixture(scope='module')
def counting(tmp_path_factory):
    """The emulator with its event counters (single-threaded: the counters are plain statics)."""
    so = str(tmp_path_factory.mktemp('emu_cnt') / 'librv_emu_cnt.so')
    root = os.path.join(EMU_DIR, '..', '..')
    subprocess.run(['g++', '-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mfma', '-shared', '-DRV_EMU_COUNT', '-I' + os.path.join(root, 'include'),
                    os.path.join(EMU_DIR, 'rv_emu.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.emu_create.restype = C.c_void_p
    lib.emu_create.argtypes = [C.POINTER(abi.rv_config), C.POINTER(abi.rv_scene)]
    return lib


def _counts(lib):
    c, d, d2 = (C.c_long * 48)(), (C.c_long * 16)(), (C.c_long * 48)()
    lib.emu_get_counts(c); lib.emu_get_dbg(d); lib.emu_get_dbg2(d2)
    return np.array(list(c)), np.array(list(d)), np.array(list(d2))


def test_fewer_run_boundaries_for_the_same_work(counting):
    """(16 envs, 4 steps, seed 1234): the substeps, the heavy substeps and the IK calls are the parent's to the last
    one; the fused coasting runs and the re-measurements of the kinematics are each at least 20 % fewer (the bound
    alone gives -23 % and -26 %); runs end on the body clearance and on the table clearance."""
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(), n_envs=16, seed=1234, shape_names=names)
    h = C.c_void_p(counting.emu_create(C.byref(cfg), C.byref(scene)))
    counting.emu_reset(h, None)
    c0, _, e0 = _counts(counting)
    counting.emu_rollout(h, 4, 0, 1)
    c1, _, e1 = _counts(counting)
    c, d2 = c1 - c0, e1 - e0
    print('fused runs %d (parent %d), re-measured %d (parent %d), fused + regular substeps %d, heavy %d, IK calls %d'
          % (c[2], PARENT_RUNS, c[12], PARENT_REMEASURED, c[3] + c[9], c[10], c[0]))
    body_limited, table_limited = int(d2[0:20:2].sum()), int(d2[1:20:2].sum())
    print('runs ended by the clearance: body-limited %d, table-limited %d' % (body_limited, table_limited))
    assert body_limited > 0 and table_limited > 0
    assert c[3] + c[9] == SUBSTEPS and c[10] == HEAVY and c[0] == IK_CALLS
    assert c[2] <= 0.8 * PARENT_RUNS, c[2]
    assert c[12] <= 0.8 * PARENT_REMEASURED, c[12]


def test_the_diagonal_scene_measures_with_three_positive_gaps(counting):
    """Slots 8 .. 11 of the emulator's debug counters (coast_measure_clearances under RV_EMU_COUNT): (box, measurement)
    pairs in which the body clearance is the smaller of the box's two, by the term that set it for the nearest body --
    the largest gap, the sqrt 3 term, the query's distance bound, and (slot 11) the sqrt 3 term with the box off the
    body along all three axes.  The diagonal scene has such measurements; and the run is still the oracle's."""
    _, a0, _ = _counts(counting)
    ref, st = run_oracle('diagonal_sleeper', N_A, SEED_A, STEPS_A)
    e = run_emu(counting, 'diagonal_sleeper', N_A, SEED_A, STEPS_A, st)
    _, a1, _ = _counts(counting)
    terms = (a1 - a0)[8:12]
    print('body clearance set by: largest gap %d, sqrt 3 term %d, distance bound %d, sqrt 3 term with three positive gaps %d' % tuple(terms))
    assert terms[3] > 0 and terms[0] > 0 and terms[2] > 0
    assert np.array_equal(e.body_state(), ref.body_state().astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# (c) the inequality

def _aabb_dist(lo_a, hi_a, lo_b, hi_b):
    g = np.maximum(np.maximum(lo_b - hi_a, lo_a - hi_b), 0.0)
    return np.sqrt((g * g).sum(-1)), g


def test_the_admissible_travel_keeps_the_aabb_distance_above_the_range():
    """This checks the inequality, not the C text ((a) above checks the C text): for random pairs of axis-aligned boxes
    and a range R, with adm = max(g_max - R, (d - R) / sqrt 3) and every face of the second box shifted by at most
    D = adm (1 - 1e-9), the AABB distance stays >= R.  In float64, on boxes of a metre and less, with adm >= 1 mm: the
    1e-12 m that D stays below adm is four orders above the rounding of the distance.  The shifts are random ones and
    the worst one (every face towards the first box by D).  And the bound is not idle: on pairs apart along one axis
    only, 1 % more travel than adm brings the distance below R."""
    rng = np.random.default_rng(5)
    n = 200000
    lo_a = rng.uniform(-0.5, 0.5, (n, 3)); hi_a = lo_a + rng.uniform(0.02, 0.3, (n, 3))
    size_b = rng.uniform(0.02, 0.3, (n, 3))
    gap = rng.uniform(-0.015, 0.25, (n, 3))                     # (negative: the boxes overlap along that axis)
    gap[rng.random((n, 3)) < 0.3] *= 0.1                        # ... and many gaps of the size of R
    above = rng.random((n, 3)) < 0.5
    lo_b = np.where(above, hi_a + gap, lo_a - gap - size_b); hi_b = lo_b + size_b
    R = rng.uniform(0.0, 0.03, n)
    d, g = _aabb_dist(lo_a, hi_a, lo_b, hi_b)
    adm = np.maximum(g.max(-1) - R, (d - R) / np.sqrt(3.0))
    use = adm >= 1e-3
    assert use.sum() > n // 4
    third = ((d - R) / np.sqrt(3.0) > g.max(-1) - R) & use
    assert third.sum() > n // 100 and ((g > 0).all(-1) & third).sum() > n // 100       # both terms are exercised
    D = (adm * (1.0 - 1e-9))[:, None]
    towards = np.where(above, -1.0, 1.0)
    for shift_lo, shift_hi in [(towards * D, towards * D)] + [(rng.uniform(-1, 1, (n, 3)) * D, rng.uniform(-1, 1, (n, 3)) * D) for _ in range(3)]:
        d1, _ = _aabb_dist(lo_a, hi_a, lo_b + shift_lo, hi_b + shift_hi)
        assert (d1[use] >= R[use]).all()
    one_axis = use & ((g > 0).sum(-1) == 1) & (R > 1e-3)
    assert one_axis.sum() > 100
    more = towards * (g > 0) * 1.01 * adm[:, None]
    d2, _ = _aabb_dist(lo_a, hi_a, lo_b + more, hi_b + more)
    assert (d2[one_axis] < R[one_axis]).all()
