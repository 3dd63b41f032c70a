"""The tail of a recorded rollout (rv_env_kernel.h, rv_pc_tail): workgroups of the plain launch of the
one-wave-per-SIMD env kernel whose env has finished render the point clouds of snapshot rows that are stored
already; the k_point_cloud launch after the kernel renders the rows they left.

Who renders a row depends on timing; what is rendered must not.  Every case compares EVERYTHING a recorded rollout
returns -- all observation tensors with the point clouds, rewards, dones -- byte for byte with the same world type run
with RV_PC_TAIL=0 (every cloud rendered after the kernel), and the point clouds with the float oracle's, stepped along
one env.step() at a time; and it asserts that every row was rendered exactly once: by_tail + by_residual == K x N.
"""
import functools

import numpy as np
import pytest

from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu


def _cfg(n, seed, **over):
    scene, names = scenes.make_scene()
    env_cfg = configs.push_env_config(**over)
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, shape_names=names), scene


def _np(x):
    if isinstance(x, dict):
        return {k: _np(v) for k, v in x.items()}
    return x.cpu().numpy()


def _device(n, seed, launches, auto_reset, over, full=False, point_cloud=True):
    """A fresh world, reset, then one recorded rollout per entry of `launches` (steps); returns per launch
    (obs, rewards, dones, extra or None, (by_tail, by_residual)) as numpy.  Reads the environment as it is."""
    from robovat_amd import lib
    cfg, scene = _cfg(n, seed, **dict(over))
    w = lib.World(cfg, scene, device=0)
    w.reset()
    out, first = [], 0
    for k in launches:
        if full:
            obs, r, d, ex = w.rollout_record_full(k, first_macro_index=first, auto_reset=auto_reset, point_cloud=point_cloud)
        else:
            obs, r, d = w.rollout_record(k, first_macro_index=first, auto_reset=auto_reset, point_cloud=point_cloud)
            ex = None
        counts = w.last_tail_renders()
        out.append((_np(obs), _np(r), _np(d), None if ex is None else _np(ex), counts))
        first += k
    build = w.env_kernel_build()
    w.close()
    return out, build


@functools.lru_cache(maxsize=None)
def _oracle_clouds(n, seed, launches, auto_reset, over):
    """[sum(launches)][N][RV_MAXB][P][3] point clouds of the float oracle after every env.step(), and [..][N] whether
    the env took that step (an env whose episode is over takes none without auto_reset: its rows are zero)."""
    from oracle import orc
    cfg, scene = _cfg(n, seed, **dict(over))
    ref = orc.OracleWorld(cfg, scene, double=False)
    ref.reset()
    clouds, stepped = [], []
    done = np.zeros(n, bool)
    for k in range(sum(launches)):
        stepped.append(np.ones(n, bool) if auto_reset else ~done)
        ref.rollout(1, k, bool(auto_reset))
        clouds.append(ref.point_cloud().copy())
        done = np.asarray(ref.reward()[1]).astype(bool)
    return np.stack(clouds), np.stack(stepped)


@functools.lru_cache(maxsize=None)
def _parent_path(n, seed, launches, auto_reset, over, full=False, occ=None):
    """The same run of the same world type (occ: RV_ENV_OCC, the build of the env kernel the world is forced onto) with
    every cloud rendered after the kernel (RV_PC_TAIL=0).  Computed once per shape and build, never changed."""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv('RV_PC_TAIL', '0')
        mp.delenv('RV_PC_TAIL_CAP', raising=False)
        if occ is None:
            mp.delenv('RV_ENV_OCC', raising=False)
        else:
            mp.setenv('RV_ENV_OCC', occ)
        out, _ = _device(n, seed, launches, auto_reset, over, full=full)
    finally:
        mp.undo()
    for rec in out:
        assert rec[4] == (0, rec[1].size)      # no tail: every row by the launch after the kernel
    return out


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            _same(a[k], b[k], what + '.' + k)
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _check(n, seed, launches, auto_reset, over, full=False, occ=None):
    """Run with the environment as the test set it; compare with the RV_PC_TAIL=0 run and with the oracle.  Returns the
    (by_tail, by_residual) of every launch."""
    over = tuple(sorted(over.items()))
    launches = tuple(launches)
    got, build = _device(n, seed, launches, auto_reset, over, full=full)
    want = _parent_path(n, seed, launches, auto_reset, over, full, occ)
    clouds, stepped = _oracle_clouds(n, seed, launches, auto_reset, over)
    first, counts = 0, []
    for i, k in enumerate(launches):
        obs, r, d, ex, c = got[i]
        _same(obs, want[i][0], 'launch %d obs' % i)
        _same(r, want[i][1], 'launch %d reward' % i)
        _same(d, want[i][2], 'launch %d done' % i)
        if full:
            _same(ex, want[i][3], 'launch %d extra' % i)
        pc = obs['point_cloud']
        assert pc.shape == (k, n, abi.RV_MAXB, pc.shape[3], 3)
        st = stepped[first:first + k]
        assert pc[st].tobytes() == clouds[first:first + k][st].tobytes(), 'launch %d: point clouds against the oracle' % i
        assert (pc[~st] == 0).all()
        assert c[0] >= 0 and c[1] >= 0 and c[0] + c[1] == k * n, c
        counts.append(c)
        first += k
    return counts, build


@pytest.mark.parametrize('k', [1, 3])
def test_one_env_renders_after_its_own_last_step(k):
    """N = 1: no helper ever exists; what the tail renders, the env's own workgroup renders after its last step."""
    counts, build = _check(1, 41, [k], True, dict(MAX_STEPS=2))
    assert build == abi.RV_ENV_BUILD_OCC1
    # deterministic: the workgroup says that all K rows are stored, then claims them itself -- nobody else is there.
    # (A tail that never recognised its own XCD's tag would leave them all to the launch after the kernel.)
    assert counts[0] == (k, 0)


def test_fewer_envs_than_xcds():
    """N = 5: some XCD holds one env or none.  Every env is alone among its candidates (env + 8 i < 5): each workgroup
    renders exactly its own K rows."""
    counts, _ = _check(5, 43, [3], True, dict(MAX_STEPS=2))
    assert counts[0] == (3 * 5, 0)


@pytest.mark.parametrize('auto_reset', [True, False])
def test_episodes_end_inside_the_launch(auto_reset):
    """N = 64, K = 4, MAX_STEPS = 2: with auto_reset the envs are reset inside the launch; without it the steps after the
    episode's end are not taken (zero rows, stored by the env's workgroup when it leaves)."""
    _check(64, 47, [4], auto_reset, dict(MAX_STEPS=2))


def test_cap_0_leaves_every_row_to_the_launch_after_the_kernel(monkeypatch):
    monkeypatch.setenv('RV_PC_TAIL_CAP', '0')
    counts, _ = _check(64, 47, [4], True, dict(MAX_STEPS=2))
    assert counts[0] == (0, 4 * 64)


def test_cap_1_mixes_tail_and_residual(monkeypatch):
    """One row per finished workgroup at most: 64 rows at most by the tail, so both renderers have work."""
    monkeypatch.setenv('RV_PC_TAIL_CAP', '1')
    counts, _ = _check(64, 47, [4], True, dict(MAX_STEPS=2))
    assert counts[0][0] > 0 and counts[0][1] > 0, counts


def test_two_launches_on_one_world():
    """K = 3 then K = 2: a done / claimed / rendered word left over from the first launch would show in the second."""
    _check(64, 53, [3, 2], True, dict(MAX_STEPS=2))


def test_without_point_clouds_no_word_is_touched():
    out, _ = _device(16, 59, (3,), True, (('MAX_STEPS', 2),), point_cloud=False)
    assert out[0][4] == (0, 0)
    assert 'point_cloud' not in out[0][0]


def test_rollout_record_full_reset_clouds_come_from_the_old_path():
    """N = 16, K = 3: the step clouds may come from the tail; the clouds after the resets are rendered after the kernel as
    ever.  Both equal the RV_PC_TAIL=0 run (the `extra` record is compared whole)."""
    _check(16, 61, [3], True, dict(MAX_STEPS=2), full=True)


def test_the_two_waves_per_simd_build_has_no_tail(monkeypatch):
    """RV_ENV_OCC=2: against the RV_PC_TAIL=0 run of a world forced onto the same build."""
    monkeypatch.setenv('RV_ENV_OCC', '2')
    counts, build = _check(64, 47, [4], True, dict(MAX_STEPS=2), occ='2')
    assert build == abi.RV_ENV_BUILD_OCC2
    assert counts[0] == (0, 4 * 64)
