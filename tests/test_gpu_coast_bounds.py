"""The body clearance of coasting (coast_measure_clearances in robovat_amd/csrc/rv_dev_env.h) on the GPU: the four
scenes of tests/test_coast_bounds_emu.py, 64 envs x 3 steps, on both builds of the env kernel against the float oracle,
bit for bit -- body states, joint states, env counters, manifold counts and link poses, no tolerance anywhere.  The
oracle never coasts: it runs the wake test of every (sleeping body, collider box) pair in every substep, so equality
says that every test a coasting run skipped would have said no.

Each scene runs as one launch of three steps and, once more, as launches of 1 and 2 steps: the clearances a run
leaves over survive the end of a launch, and the next launch goes on with them.  The oracle's state does not depend on
the cut; the env counters from column 7 on hold the last launch only, so the cut run compares the columns [:7].

The oracle's side of a scene is computed once per module and is read-only afterwards.
"""
import numpy as np
import pytest

from test_kat_contact import _Np
from test_gpu_env_builds import _freeze, _same, _state, make_world   # noqa: F401  (make_world: the fixture, both builds)
from test_coast_bounds_emu import SCENES, make_case, run_oracle

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 64, 3, 4


@pytest.fixture(scope='module')
def oracle_runs():
    done = {}

    def get(name):
        if name not in done:
            ref, st = run_oracle(name, N, SEED, STEPS)
            assert ref.stats()['env_steps'] == N * STEPS
            done[name] = _freeze(dict(state=_state(ref), set_state=st))
        return done[name]
    return get


@pytest.mark.parametrize('launches', [(3,), (1, 2)], ids=['one_launch', 'launches_of_1_and_2'])
@pytest.mark.parametrize('name', SCENES)
def test_scene_equals_the_float_oracle(make_world, oracle_runs, name, launches):
    want = oracle_runs(name)
    w = _Np(make_world(*make_case(name, N, SEED)))
    w.reset()
    if want['set_state'] is not None:
        w.set_body_state(np.array(want['set_state'])); w.wait_until_stable()      # (a copy: the shared one is read-only)
    k = 0
    for c in launches:
        w.rollout(c, k, True)
        k += c
    _same(_state(w), want['state'], '%s, launches %s' % (name, launches), counters=None if len(launches) == 1 else 7)
