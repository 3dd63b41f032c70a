"""rv_render_view, record_step and the RECORDING option on the device (MI355X).

Small worlds throughout (2 to 4 envs); every comparison is bit for bit except the one against the float64 ray caster of
tests/camera_host.py, whose bounds are explained at DEPTH_BOUND."""
import ctypes as C

import numpy as np
import pytest

from robovat_amd import abi, configs
from robovat_amd.perception import camera_row

import camera_host as ch
import render_view_host as rvh
from test_camera_host import render_case

pytestmark = pytest.mark.gpu

CASES = ['push', 'concave', 'grasp']
BACKGROUND = (30, 30, 30)      # shade_rgb's colour of "nothing hit"

# Largest |depth - float64 ray cast| over the agreeing pixels of the free views below (four views x two envs per case),
# in metres of eye depth.  Two sets of figures for the float ORACLE rendering these views as config cameras on the CPU:
#   as the issue that asked for this test states them: 1.2e-5 with convex templates, 5.7e-5 with concave ones (top view,
#     env 1) -- against the default view's 1.9e-6 / 1.2e-5 (tests/test_camera_host.py);
#   as measured with the views of tests/render_view_host.py (principal point ((W - 1) / 2, (H - 1) / 2)): 5.1e-6 convex
#     (push, view 1, env 1) and 1.6e-5 concave (top view, env 1).  One figure repeats in every case, 2.6e-6 in view 1:
#     its pixel carries label RV_MAXB + 1 -- the static piece behind it is the ARM (its link boxes stand the same way
#     after every reset), not the table.
# The bounds are the project's 4 x the first set: 4.8e-5 and 2.3e-4.  The test prints what the device measures.
DEPTH_BOUND = {'push': 4.8e-5, 'grasp': 4.8e-5, 'concave': 2.3e-4}


def _np(t):
    return t.cpu().numpy()


def _world(name, n):
    from robovat_amd import lib
    cfg, scene, _ = render_case(name, n=n)
    w = lib.World(cfg, scene, device=0)
    w.reset()
    return w, cfg, scene


def _step(w, k=0):
    w.set_actions(w.policy_random(k))
    w.step_macro()


def _view_cams(cfg):
    return rvh.free_views(cfg, float(cfg.table_z))


# ---------------------------------------------------------------- 1. own camera == the existing renders
@pytest.mark.parametrize('name', CASES)
def test_own_cameras_reproduce_render_and_render_rgb(name):
    """views = the rows of World.camera(), all envs, the config's size: rgb, depth and segmask equal render_rgb() /
    render() bit for bit, after reset and after one step"""
    w, cfg, _ = _world(name, 3)
    for moment in ('reset', 'step'):
        if moment == 'step':
            _step(w)
        out = w.render_view(w.camera(), rgb=True, depth=True, segmask=True)
        depth, seg = w.render()
        rgb = w.render_rgb()
        assert tuple(out['rgb'].shape) == (3, int(cfg.cam_height), int(cfg.cam_width), 3)
        assert np.array_equal(_np(out['rgb']), _np(rgb)), moment
        assert np.array_equal(_np(out['depth']).view(np.uint32), _np(depth).view(np.uint32)), moment
        assert np.array_equal(_np(out['segmask']), _np(seg)), moment
        assert len(np.unique(_np(seg))) >= 4      # bodies, table, arm: not an empty picture
    w.close()


# ---------------------------------------------------------------- 2. free views against the float64 ray caster
@pytest.mark.parametrize('name', CASES)
def test_free_views_vs_independent_ray_cast(name):
    """four views per env (tests/render_view_host.py: from three sides and from above, 120 x 160, f = 0.9 W) against
    camera_host.raycast of the device's own state through a config copy with the view's size: the same label on every
    pixel the ray caster decides, at most 0.2 % undecided, every label the reference shows among the compared pixels --
    and, over the four views of an env, the table, the arm and every active body --, depth within DEPTH_BOUND"""
    w, cfg, scene = _world(name, 2)
    cams = _view_cams(cfg)
    rows = np.stack([camera_row(c) for c in cams])
    idx = np.repeat(np.arange(2), len(cams))
    out = w.render_view(np.tile(rows, (2, 1)), idx, rvh.VIEW_H, rvh.VIEW_W, rgb=False, depth=True, segmask=True)
    depth, seg = _np(out['depth']), _np(out['segmask'])
    st, bp, lp = _np(w.body_state()), _np(w.body_params()), _np(w.link_poses())
    small = type(cfg).from_buffer_copy(cfg)
    small.cam_height, small.cam_width = rvh.VIEW_H, rvh.VIEW_W
    worst = 0.0
    for i in range(2):
        shown = set()
        for k in range(len(cams)):
            v = i * len(cams) + k
            ref = ch.raycast(small, scene, st[i], bp[i], lp[i], ch.camera_of(small, rows[k]))
            present = sorted(set(ref[1][~ref[2]].tolist()) - {255})
            err, share = ch.compare_render(depth[v], seg[v], ref, present)
            print('%s env %d view %d: max |depth - ray cast| %.3e m, undecided pixels %.3f %%, labels %s' % (name, i, k, err, 100 * share, present))
            assert err <= DEPTH_BOUND[name], (err, DEPTH_BOUND[name])
            worst = max(worst, err)
            shown |= set(present)
        need = {b for b in range(abi.RV_MAXB) if bp[i][b][0]} | {abi.RV_MAXB, abi.RV_MAXB + 1}
        assert need <= shown, (need, shown)
    print('%s: largest depth difference %.3e m (bound %.1e)' % (name, worst, DEPTH_BOUND[name]))
    w.close()


# ---------------------------------------------------------------- 3. a row depends on its own (camera, env) only
def test_a_view_depends_on_its_own_camera_and_env_only():
    """V = 1 on env N - 1, several cameras on one env and a permuted index list: every row equals the row rendered alone"""
    w, cfg, _ = _world('push', 3)
    H, W = 24, 32
    rows = np.stack([camera_row(c) for c in rvh.free_views(cfg, float(cfg.table_z), H, W)])

    def one(r, i):
        o = w.render_view(rows[r], [i], H, W, rgb=True, depth=True, segmask=True)
        return [_np(o[k])[0] for k in ('rgb', 'depth', 'segmask')]

    def many(rs, idx):
        o = w.render_view(rows[list(rs)], list(idx), H, W, rgb=True, depth=True, segmask=True)
        return [_np(o[k]) for k in ('rgb', 'depth', 'segmask')]

    alone = {(r, i): one(r, i) for r in range(4) for i in range(3)}
    assert not np.array_equal(alone[(0, 0)][0], alone[(0, 1)][0]) and not np.array_equal(alone[(0, 2)][0], alone[(1, 2)][0])
    for rs, idx in (((2,), (2,)),                                       # V = 1 on the last env
                    ((0, 1, 2, 3), (1, 1, 1, 1)),                       # four cameras on one env
                    ((0, 1, 2, 3, 0, 1), (2, 0, 1, 0, 1, 2)),           # a permuted index list
                    ((3, 3, 3), (2, 1, 0))):                            # one camera, the envs backwards
        got = many(rs, idx)
        for v, (r, i) in enumerate(zip(rs, idx)):
            for g, want in zip(got, alone[(r, i)]):
                assert np.array_equal(g[v], want), (rs, idx, v)
    # the Python conveniences: one Camera broadcast over the envs, env_index None = all envs, the camera's own size
    o = w.render_view(rvh.free_views(cfg, float(cfg.table_z), H, W)[1])
    assert tuple(o['rgb'].shape) == (3, H, W, 3) and sorted(o) == ['rgb']
    for i in range(3):
        assert np.array_equal(_np(o['rgb'])[i], alone[(1, i)][0])
    w.close()


# ---------------------------------------------------------------- 4. supersampling
@pytest.mark.parametrize('size', [(24, 32), (23, 31)])
def test_supersampling_is_the_integer_box_filter(size):
    """render_view(s) == box filter of render_view(1) at (s H, s W) with the scaled row, bit for bit, for s = 2, 3, 4;
    where the segmask says 255 the rgb is the background colour"""
    H, W = size
    w, cfg, _ = _world('push', 2)
    rows = np.stack([camera_row(c) for c in rvh.free_views(cfg, float(cfg.table_z), H, W)])
    idx = [0, 1, 1, 0]
    base = w.render_view(rows, idx, H, W, rgb=True, segmask=True)
    rgb1, seg1 = _np(base['rgb']), _np(base['segmask'])
    assert (seg1 == 255).any() and (seg1 != 255).any()
    assert (rgb1[seg1 == 255] == np.array(BACKGROUND, np.uint8)).all()
    assert np.array_equal(_np(w.render_view(rows, idx, H, W, supersample=1)['rgb']), rgb1)
    for s in (2, 3, 4):
        got = _np(w.render_view(rows, idx, H, W, supersample=s)['rgb'])
        hi = _np(w.render_view(rvh.scaled_row(rows, s), idx, s * H, s * W)['rgb'])
        assert got.shape == (4, H, W, 3) and hi.shape == (4, s * H, s * W, 3)
        assert np.array_equal(got, rvh.box_filter(hi, s)), s
        assert not np.array_equal(got, rgb1)      # (edges are blended: it is not the s = 1 picture)
    w.close()


# ---------------------------------------------------------------- 5. edges of the launch
@pytest.mark.parametrize('size', [(1, 1), (7, 13)])
def test_launch_edges_guard_words_odd_offsets_and_slices(size):
    """sizes that fill no workgroup; guard bytes around every output stay; an rgb pointer at an odd byte offset; outputs
    that are slices of larger tensors"""
    import torch
    H, W = size
    V = 3
    w, cfg, _ = _world('push', 2)
    rows = np.stack([camera_row(c) for c in rvh.free_views(cfg, float(cfg.table_z), H, W)])[:V]
    idx = [1, 0, 1]
    want = w.render_view(rows, idx, H, W, rgb=True, depth=True, segmask=True)
    n = V * H * W
    G = 64
    flat = torch.full((G + 1 + 3 * n + G,), 0xA5, dtype=torch.uint8, device=w.device)
    rgb = flat[G + 1: G + 1 + 3 * n].view(V, H, W, 3)
    assert rgb.data_ptr() % 2 == 1 and rgb.is_contiguous()
    big_d = torch.full((V + 4, H, W), -7.0, dtype=torch.float32, device=w.device)
    big_s = torch.full((V + 4, H, W), 0x5A, dtype=torch.uint8, device=w.device)
    got = w.render_view(rows, idx, H, W, out={'rgb': rgb, 'depth': big_d[2:2 + V], 'segmask': big_s[2:2 + V]})
    assert got['rgb'] is rgb
    for k in ('rgb', 'depth', 'segmask'):
        assert np.array_equal(_np(got[k]), _np(want[k])), k
    f = _np(flat)
    assert (f[:G + 1] == 0xA5).all() and (f[G + 1 + 3 * n:] == 0xA5).all()
    assert (_np(big_d[:2]) == -7.0).all() and (_np(big_d[2 + V:]) == -7.0).all()
    assert (_np(big_s[:2]) == 0x5A).all() and (_np(big_s[2 + V:]) == 0x5A).all()
    w.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched():
    """every refusal of include/rovat.h returns RV_ERR_VALUE (ValueError through lib.check) and writes nothing; the largest
    legal supersample and a 4096-wide single-row view run"""
    import torch
    from robovat_amd import lib
    w, cfg, _ = _world('push', 2)
    H, W, V = 6, 8, 2
    rows = np.ascontiguousarray(np.stack([camera_row(c) for c in rvh.free_views(cfg, float(cfg.table_z), H, W)])[:V])
    idx = np.array([0, 1], np.int32)
    rgb = torch.full((V, H, W, 3), 0xA5, dtype=torch.uint8, device=w.device)
    depth = torch.full((V * H * W + 1,), -7.0, dtype=torch.float32, device=w.device)
    seg = torch.full((V, H, W), 0x5A, dtype=torch.uint8, device=w.device)
    vp = C.c_void_p

    def call(p=None, idx_=idx, rows_=rows, rgb_=rgb.data_ptr(), depth_=None, seg_=None, null=()):
        p = p if p is not None else abi.rv_view_params(V, H, W, 1)
        return w.lib.rv_render_view(w.h, None if 'p' in null else C.byref(p),
                                    None if 'idx' in null else idx_.ctypes.data_as(vp),
                                    None if 'rows' in null else rows_.ctypes.data_as(vp),
                                    None if rgb_ is None else vp(rgb_), None if depth_ is None else vp(depth_),
                                    None if seg_ is None else vp(seg_))

    def bad_row(j, value):
        r = rows.copy()
        r[1, j] = value
        return r

    refused = [
        dict(null=('p',)), dict(null=('idx',)), dict(null=('rows',)),
        dict(rgb_=None),
        dict(p=abi.rv_view_params(0, H, W, 1)), dict(p=abi.rv_view_params(4097, H, W, 1)), dict(p=abi.rv_view_params(-1, H, W, 1)),
        dict(p=abi.rv_view_params(V, 0, W, 1)), dict(p=abi.rv_view_params(V, 4097, W, 1)),
        dict(p=abi.rv_view_params(V, H, 0, 1)), dict(p=abi.rv_view_params(V, H, 4097, 1)),
        dict(p=abi.rv_view_params(V, H, W, 0)), dict(p=abi.rv_view_params(V, H, W, 5)),
        dict(idx_=np.array([0, 2], np.int32)), dict(idx_=np.array([-1, 0], np.int32)),
        dict(rows_=bad_row(7, np.nan)), dict(rows_=bad_row(16, np.inf)), dict(rows_=bad_row(2, -np.inf)),
        dict(rows_=bad_row(0, 0.0)), dict(rows_=bad_row(1, 0.0)),
        dict(depth_=depth.data_ptr() + 2), dict(depth_=depth.data_ptr() + 1, rgb_=None),
        dict(p=abi.rv_view_params(V, H, W, 2), depth_=depth.data_ptr()), dict(p=abi.rv_view_params(V, H, W, 2), seg_=seg.data_ptr()),
    ]
    for kw in refused:
        rc = call(**kw)
        assert rc == abi.RV_ERR_VALUE, kw
        with pytest.raises(ValueError):
            lib.check(rc)
    w.synchronize()
    assert (_np(rgb) == 0xA5).all() and (_np(depth) == -7.0).all() and (_np(seg) == 0x5A).all()
    # the Python layer refuses the same before it gets there
    for kw in (dict(supersample=5), dict(height=0), dict(supersample=2, depth=True), dict(env_index=[0, 2])):
        args = dict(cameras=rows, env_index=[0, 1], height=H, width=W)
        args.update(kw)
        with pytest.raises(ValueError):
            w.render_view(**args)
    with pytest.raises(ValueError):
        w.render_view(rows, [0, 1], H, W, out={'rgb': rgb[:, :, :, :2]})
    with pytest.raises(ValueError):
        w.render_view(np.tile(rows, (2, 1))[:3], None, H, W)      # three cameras, two envs, no index
    # what is legal runs: everything at once, the largest supersample, a 4096-wide single row
    assert call(depth_=depth.data_ptr(), seg_=seg.data_ptr()) == abi.RV_OK
    assert not (_np(rgb) == 0xA5).all() and not (_np(depth)[:-1] == -7.0).any() and float(depth[-1]) == -7.0
    s4 = _np(w.render_view(rows, idx, H, W, supersample=abi.RV_VIEW_MAX_SUPERSAMPLE)['rgb'])
    hi = _np(w.render_view(rvh.scaled_row(rows, 4), idx, 4 * H, 4 * W)['rgb'])
    assert np.array_equal(s4, rvh.box_filter(hi, 4))
    wide_rows = np.stack([camera_row(c) for c in rvh.free_views(cfg, float(cfg.table_z), 1, abi.RV_VIEW_MAX_SIDE)])[:1]
    wide = w.render_view(wide_rows, [1], 1, abi.RV_VIEW_MAX_SIDE, rgb=True, segmask=True)
    assert tuple(wide['rgb'].shape) == (1, 1, 4096, 3) and len(np.unique(_np(wide['segmask']))) >= 2
    w.close()


# ---------------------------------------------------------------- 7. state
def test_render_view_leaves_the_envs_alone():
    """save_state() bytes are the same before and after render_view -- also in the middle of a partial step, which goes
    on afterwards as if nobody had looked"""
    w, cfg, _ = _world('push', 2)
    twin, _, _ = _world('push', 2)
    cams = rvh.free_views(cfg, float(cfg.table_z), 24, 32)
    before = _np(w.save_state().blocks)
    w.render_view(cams, [0, 1, 1, 0], supersample=2)
    assert np.array_equal(_np(w.save_state().blocks), before)
    a = w.policy_random(0)
    for x in (w, twin):
        x.step_begin(a)
        assert not _np(x.step_poll(max_substeps=60)).any()
    mid = _np(w.save_state().blocks)
    assert not np.array_equal(mid, before)
    w.render_view(cams, [0, 1, 1, 0], rgb=True, depth=True, segmask=True)
    assert np.array_equal(_np(w.save_state().blocks), mid)
    for x in (w, twin):
        assert _np(x.step_poll()).all()
    for get in ('body_state', 'joint_state', 'link_poses', 'manifold_counts'):
        assert np.array_equal(_np(getattr(w, get)()), _np(getattr(twin, get)())), get
    assert np.array_equal(_np(w.env_counters())[:, :7], _np(twin.env_counters())[:, :7])
    a, b = _np(w.save_state().blocks).view(np.uint32), _np(twin.save_state().blocks).view(np.uint32)
    print('words of the env blocks that differ from the twin that was not looked at: %s' % np.argwhere(a != b).tolist()[:16])
    w.close(); twin.close()


# ---------------------------------------------------------------- 8. record_step
def _same_obs(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = (a[k], b[k])
        x = _np(x) if hasattr(x, 'cpu') else np.asarray(x)
        y = _np(y) if hasattr(y, 'cpu') else np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _check_record(env, twin, actions, cams, rows_of, every, max_frames=256):
    """env.record_step against twin.step and against renders of env before / after; returns the record"""
    world = env.world
    v = len(rows_of)
    h, w = int(cams[0].height), int(cams[0].width)
    first = _np(world.render_view(cams, rows_of)['rgb'])
    obs, reward, done, rec = env.record_step(actions, cams, rows_of, every, max_frames=max_frames)
    want = twin.step(actions)
    _same_obs(obs, want[0])
    assert np.array_equal(_np(reward).view(np.uint32), _np(want[1]).view(np.uint32)) and np.array_equal(_np(done), _np(want[2]))
    assert want[3] is None
    assert np.array_equal(_np(env.save_state().blocks), _np(twin.save_state().blocks))
    assert env.stats() == twin.stats() and env._macro_index == twin._macro_index
    t = rec['num_frames']
    frames, stamps = _np(rec['frames']), _np(rec['sim_steps'])
    assert frames.shape == (t, v, h, w, 3) and stamps.shape == (t, v) and 2 <= t <= max_frames
    assert np.array_equal(frames[0], first)
    assert np.array_equal(frames[-1], _np(world.render_view(cams, rows_of)['rgb']))
    steps = np.diff(stamps.astype(np.int64), axis=0)
    assert (steps >= 0).all()
    if t < max_frames:      # (every poll was watched)
        assert (steps <= every).all(), (steps.max(), every)
        # a poll takes the substeps it is asked for or one more (record_step asks for every - 1): an env that
        # does not finish in a poll moves on by every - 1 or every, and only its last poll may take fewer
        for k in range(v):
            moving = np.nonzero(steps[:, k])[0]
            assert (steps[moving[:-1], k] >= every - 1).all(), (k, steps[:, k])
    assert np.array_equal(stamps[-1], _np(world.env_counters())[rows_of, 0])
    return frames, stamps


def test_record_step_push():
    """VecPushEnv.record_step, N = 4, views on envs 1 and 3 at 48 x 64: observation, reward, done, state bytes and stats
    are a twin's step(); frame 0 / the last frame are renders of the env before / after; the stamps advance by at most `every`;
    a finished env's frames repeat and a moving arm shows; a max_frames too small still completes the same step"""
    from robovat_amd.envs.push.push_env import VecPushEnv
    envs = [VecPushEnv(4, seed=4) for _ in range(4)]
    env, twin, short, probe = envs
    for e in envs:
        e.reset()
    cfg = env.rv_config
    cams = rvh.free_views(cfg, float(cfg.table_z), 48, 64)[:2]
    rows_of = [1, 3]
    a0 = env.sample_random_actions()
    probe.step(a0)
    sub = _np(probe.world.env_counters())[rows_of, 7]
    every = int(max(sub.max() // 14, 1))      # 15 or 16 frames of the slower env
    print('substeps of envs 1 and 3: %s, every = %d' % (sub.tolist(), every))
    frames, stamps = _check_record(env, twin, a0, cams, rows_of, every)
    print('frames %d, stamps of the last three: %s' % (len(frames), stamps[-3:].tolist()))
    assert 8 <= len(frames) <= 30
    assert (np.diff(stamps[:, 0]) > 0).any() and stamps[-1, 0] - stamps[0, 0] == sub[0] and stamps[-1, 1] - stamps[0, 1] == sub[1]
    for k in range(2):
        t_end = int(np.nonzero(np.diff(stamps[:, k]))[0].max()) + 1      # the frame at which env k had finished
        for t in range(t_end, len(frames)):
            assert np.array_equal(frames[t, k], frames[t_end, k])
        assert len({frames[t, k].tobytes() for t in range(len(frames))}) >= 2      # the arm moved
    if abs(int(sub[0]) - int(sub[1])) > every:      # one env finished a whole poll earlier: its image repeats
        fast = int(np.argmin(sub))
        assert stamps[-2, fast] == stamps[-1, fast] and np.array_equal(frames[-1, fast], frames[-2, fast])
    # too few frames: the step completes all the same, with the same result (the second step of the episode)
    a1 = env.sample_random_actions()
    f1, s1 = _check_record(env, twin, a1, cams, rows_of, every, max_frames=256)
    obs_s = short.record_step(a0, cams, rows_of, every, max_frames=4)
    assert obs_s[3]['num_frames'] == 4 and np.array_equal(_np(obs_s[3]['frames'])[[0, -1]], frames[[0, -1]])
    short.record_step(a1, cams, rows_of, every, max_frames=2)
    assert np.array_equal(_np(short.save_state().blocks), _np(env.save_state().blocks))
    # several views of one env, and refusals
    o = env.record_step(env.sample_random_actions(), cams, [2, 2], every * 4, supersample=2, max_frames=6)
    twin.step(twin.sample_random_actions())
    assert np.array_equal(_np(env.save_state().blocks), _np(twin.save_state().blocks)) and o[3]['num_frames'] <= 6
    assert not np.array_equal(_np(o[3]['frames'])[0, 0], _np(o[3]['frames'])[0, 1])
    for kw in (dict(every=1), dict(max_frames=1), dict(env_index=[0, 4])):
        args = dict(actions=a0, cameras=cams, env_index=rows_of, every=every)
        args.update(kw)
        with pytest.raises(ValueError):
            env.record_step(**args)
    for e in envs:
        e.close()


def test_record_step_grasp_and_the_scalar_envs():
    """VecGrasp4DofEnv.record_step, N = 2, against a twin's step(); PushEnv / Grasp4DofEnv.record_step are row 0"""
    from robovat_amd.envs.grasp.grasp_4dof_env import Grasp4DofEnv, VecGrasp4DofEnv
    from robovat_amd.envs.push.push_env import PushEnv
    env, twin = VecGrasp4DofEnv(2, seed=4), VecGrasp4DofEnv(2, seed=4)
    env.reset(); twin.reset()
    cams = rvh.free_views(env.rv_config, float(env.rv_config.table_z), 48, 64)[:1]
    a = env.sample_random_actions()
    frames, stamps = _check_record(env, twin, a, cams, [1, 0], 150)
    print('grasp: %d frames, substeps %s' % (len(frames), (stamps[-1] - stamps[0]).tolist()))
    assert len(frames) >= 3 and len({frames[t, 0].tobytes() for t in range(len(frames))}) >= 2
    env.close(); twin.close()
    for cls in (PushEnv, Grasp4DofEnv):
        one, two = cls(seed=4), cls(seed=4)
        one.reset(); two.reset()
        act = one.action_space.sample() if cls is PushEnv else _np(one._vec.sample_random_actions())[0]
        cam = rvh.free_views(one._vec.rv_config, float(one._vec.rv_config.table_z), 24, 32)[0]
        obs, reward, done, rec = one.record_step(act, cam, 400, max_frames=8)
        obs2, reward2, done2, none = two.step(act)
        _same_obs(obs, obs2)
        assert reward == reward2 and done == done2 and none is None and one.episode_reward == two.episode_reward
        assert np.array_equal(_np(one._vec.save_state().blocks), _np(two._vec.save_state().blocks))
        assert tuple(rec['frames'].shape) == (rec['num_frames'], 1, 24, 32, 3) and 2 <= rec['num_frames'] <= 8
        assert np.array_equal(_np(rec['frames'])[-1, 0], _np(one._vec.world.render_view(cam, [0])['rgb'])[0])
        one.close(); two.close()


# ---------------------------------------------------------------- 9. the RECORDING option
def _recording(tmp_path, cam, envs, fmt='png'):
    return {'USE': True, 'NUM_STEPS': 500, 'FPS': 20, 'OUTPUT_DIR': str(tmp_path), 'ENVS': envs, 'SUPERSAMPLE': 1, 'FORMAT': fmt,
            'CAMERA': {'HEIGHT': int(cam.height), 'WIDTH': int(cam.width), 'INTRINSICS': np.asarray(cam.intrinsics).tolist(),
                       'TRANSLATION': np.asarray(cam.translation).tolist(), 'ROTATION': np.asarray(cam.rotation).tolist()}}


def test_recording_option_writes_one_file_per_env_and_episode(tmp_path):
    """RECORDING.USE with ENVS = [0, 2]: two episodes write four files; their frames are those record_step gives a twin
    built without the key, frame for frame; the recorded env's outputs and state bytes are the twin's; and an env built
    without the key steps exactly as the bare world does"""
    import os
    from robovat_amd import lib, scenes
    from robovat_amd.envs.push.push_env import VecPushEnv
    from robovat_amd.io.video_utils import read_frames
    base = configs.push_env_config(MAX_STEPS=2)
    cam = rvh.free_views(configs.make_rv_config(env_cfg=base, n_envs=1), 0.0, 36, 48)[0]
    rec_cfg = configs.push_env_config(MAX_STEPS=2, RECORDING=_recording(tmp_path, cam, [0, 2]))
    env, twin, plain = VecPushEnv(3, config=rec_cfg, seed=4), VecPushEnv(3, config=base, seed=4), VecPushEnv(3, config=base, seed=4)
    assert env._recorder is not None and twin._recorder is None
    scene, names = scenes.make_scene()
    bare = lib.World(configs.make_rv_config(base, None, names, n_envs=3, seed=4), scene, device=0)
    want = {0: [[], []], 2: [[], []]}
    for episode in range(2):
        _same_obs(env.reset(), twin.reset())
        plain.reset(); bare.reset()
        for k in range(2):
            a = twin.sample_random_actions()
            got = env.step(a)
            ref = twin.record_step(a, cam, [0, 2], 500)
            _same_obs(got[0], ref[0])
            assert np.array_equal(_np(got[1]), _np(ref[1])) and np.array_equal(_np(got[2]), _np(ref[2])) and got[3] is None
            assert np.array_equal(_np(env.save_state().blocks), _np(twin.save_state().blocks))
            fr = _np(ref[3]['frames'])
            for j, i in enumerate((0, 2)):
                want[i][episode].append(fr[(1 if k else 0):, j])
            # without the key: today's step, which is these four calls on the world
            out = plain.step(a)
            bare.set_actions(a); bare.step_macro()
            _same_obs(out[0], bare.observe(point_cloud=False))
            r, d = bare.reward()
            assert np.array_equal(_np(out[1]), _np(r)) and np.array_equal(_np(out[2]), _np(d).astype(bool)) and out[3] is None
            assert np.array_equal(_np(plain.save_state().blocks), _np(bare.save_state().blocks))
            assert np.array_equal(_np(plain.save_state().blocks), _np(env.save_state().blocks))
        assert bool(got[2].all())      # MAX_STEPS = 2: the episode is over
    env.close()
    sub = os.path.join(str(tmp_path), 'data_collection')
    assert sorted(os.listdir(sub)) == ['env0_ep0000.png', 'env0_ep0001.png', 'env2_ep0000.png', 'env2_ep0001.png']
    assert [os.path.basename(p) for p in env._recorder.paths] == ['env0_ep0000.png', 'env2_ep0000.png', 'env0_ep0001.png', 'env2_ep0001.png']
    for i in (0, 2):
        for episode in range(2):
            frames, fps = read_frames(os.path.join(sub, 'env%d_ep%04d.png' % (i, episode)))
            expect = np.concatenate(want[i][episode])
            assert fps == 20.0 and frames.shape == expect.shape and len(frames) >= 4
            assert np.array_equal(frames[0], expect[0]) and np.array_equal(frames, expect)
    twin.close(); plain.close(); bare.close()
