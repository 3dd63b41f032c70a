"""rv_segment_cloud / rv_deproject without a GPU: the NumPy restatement of csrc/rv_dev_segment.h
(tests/segment_host.py) against scikit-learn's own labels (tests/golden/segment_golden.json), against float64 recounts and
the contract of group_by_labels, the counter domains of its Philox words, the host mirrors of perception/point_cloud_utils,
the bindings, and the whole chain on the float oracle's render of the push scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import segment_cases as sc
import segment_host as sh
from robovat_amd import abi, lib
from robovat_amd.perception import point_cloud_utils as pcu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN, GOLDEN_META = sc.golden()
SEED = 0x1234567855AA33CC


def test_stream_id_and_constants_match_the_headers():
    math_h = open(os.path.join(ROOT, 'robovat_amd', 'csrc', 'rv_dev_math.h')).read()
    assert int(re.search(r'#define RV_STREAM_PC\s+(\d+)u', math_h).group(1)) == sh.RV_STREAM_PC
    rovat = open(os.path.join(ROOT, 'include', 'rovat.h')).read()
    for name, value in (('RV_SEG_MAXPTS', sh.MAXPTS), ('RV_SEG_INVALID', sh.INVALID), ('RV_SEG_PLANE', sh.PLANE),
                        ('RV_SEG_SKIPPED', sh.SKIPPED), ('RV_SEG_FLAG_OVERFLOW', sh.FLAG_OVERFLOW), ('RV_SEG_FLAG_FEWER', sh.FLAG_FEWER),
                        ('RV_SEG_FLAG_NO_PLANE', sh.FLAG_NO_PLANE), ('RV_MAXB', sh.RV_MAXB)):
        assert int(re.search(r'#define %s\s+\(?(-?\d+)\)?' % name, rovat).group(1)) == value == getattr(abi, name), name
    seg_h = open(os.path.join(ROOT, 'robovat_amd', 'csrc', 'rv_dev_segment.h')).read()
    for name, value in (('RV_SEG_HYP_CTR', sh.HYP_CTR), ('RV_SEG_KEY_CTR', sh.KEY_CTR), ('RV_SEG_DRAW_CTR', sh.DRAW_CTR)):
        assert int(re.search(r'#define %s\s+(0x[0-9a-f]+)u' % name, seg_h).group(1), 16) == value


# ---- 1. DBSCAN against scikit-learn's labels
def _margin(lattice):
    d = lattice[:, None, :] - lattice[None, :, :]
    d2 = (d * d).sum(-1).astype(np.float64) / GOLDEN_META['lattice'] ** 2
    return float(np.abs(d2 - GOLDEN_META['eps'] ** 2).min())


def test_golden_cases_are_the_ones_the_issue_names():
    names = [c['name'] for c in GOLDEN]
    assert {'two_blobs_border', 'chain', 'all_noise', 'exact_min_samples', 'duplicates', 'masked_bridge', 'too_few'} <= set(names)
    by = {c['name']: c for c in GOLDEN}
    assert all(len(c['points']) <= 400 for c in GOLDEN) and GOLDEN_META['eps'] == sc.EPS
    assert len(by['chain']['points']) == 200 and by['chain']['labels'].max() == 0 and (by['chain']['labels'] == 0).all()
    assert len(by['masked_bridge']['points']) == 384 and int(by['masked_bridge']['valid'].sum()) == 383
    assert (by['all_noise']['labels'] == -1).all() and (by['too_few']['labels'] == -1).all()
    b = by['two_blobs_border']
    assert b['labels'][0] == 0 and b['labels'][-1] == 0 and set(b['labels'][1:28]) == {0} and set(b['labels'][28:55]) == {1}


@pytest.mark.parametrize('case', GOLDEN, ids=[c['name'] for c in GOLDEN])
def test_dbscan_restatement_equals_sklearn(case):
    assert _margin(case['lattice']) > GOLDEN_META['margin'] == 4e-7
    ok = np.ones(len(case['points']), bool) if case['valid'] is None else case['valid'] != 0
    lab, ncl = sh.dbscan(case['points'][ok], sc.EPS, case['min_samples'])
    assert np.array_equal(lab, case['labels']) and ncl == case['labels'].max() + 1
    # and through the whole call, with the mask: invalid points get RV_SEG_INVALID, nothing is removed with T = 0
    r = sh.segment(case['points'], case['valid'], sc.params(num_hypotheses=0, min_samples=case['min_samples']), SEED, 3)
    assert np.array_equal(r['labels'][ok], case['labels']) and (r['labels'][~ok] == sh.INVALID).all()
    assert r['info'][abi.RV_SEG_INFO_VALID] == ok.sum() and r['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_NO_PLANE


@pytest.mark.parametrize('case', [c for c in GOLDEN if c['min_samples'] == 50 or c['name'] in ('chain', 'two_blobs_border')],
                         ids=lambda c: c['name'])
def test_host_dbscan_equals_sklearn(case):
    ok = np.ones(len(case['points']), bool) if case['valid'] is None else case['valid'] != 0
    assert np.array_equal(pcu.dbscan_labels(case['points'][ok], sc.EPS, case['min_samples']), case['labels'])
    if case['min_samples'] == 50:
        assert np.array_equal(pcu.cluster(case['points'][ok], 4, method='dbscan'), case['labels'])


def test_host_cluster_methods():
    g, lab = sc.grouping_cloud()
    big = np.concatenate([sc.dense_blob((10, 10, 10), 60), sc.dense_blob((200, 200, 200), 70)])
    assert np.array_equal(pcu.cluster(big, 2, method='dbscan'), np.repeat([0, 1], [60, 70]))
    with pytest.raises(ValueError):
        pcu.cluster(big, 2, method='nope')
    try:
        import sklearn  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match='scikit-learn'):
            pcu.cluster(big, 2, method='agg')
    else:
        agg = pcu.cluster(big, 2, method='agg')
        assert len(set(agg[:60])) == 1 and len(set(agg[60:])) == 1 and agg[0] != agg[-1]
    ids = pcu.segment_by_ids(big, np.repeat([7, 9], [60, 70]), [9, 5, 7], 8)
    assert ids.shape == (3, 8, 3) and (ids[1] == 0).all() and (ids[0] > 0.15).all() and (ids[2] < 0.05).all()


# ---- 2. the plane
def test_plane_removes_exactly_the_band():
    pts, dist = sc.plane_cloud()
    assert len(pts) >= 1500 + 2 and float(np.abs(np.abs(dist) - sc.THRESH).min()) > 1e-4
    p = sc.params(min_samples=20, num_clusters=2, num_points=64)
    r = sh.segment(pts, None, p, SEED, 0)
    band = np.abs(dist) <= sc.THRESH
    assert np.array_equal(r['labels'] == sh.PLANE, band)
    assert r['info'][abi.RV_SEG_INFO_PLANE] == band.sum() and not r['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_NO_PLANE
    # the float64 recount of every hypothesis: the winner is the smallest h among the maxima
    o = sh.words(SEED, 0, 0, sh.hyp_ctr(np.arange(50)))
    ranks = np.stack([sh.mulhi(o[k], len(pts)) for k in range(3)], axis=1).astype(np.int64)
    p64 = pts.astype(np.float64)
    score = np.full(50, -1)
    for h, (a, b, c) in enumerate(ranks):
        nv = np.cross(p64[b] - p64[a], p64[c] - p64[a])
        if len({a, b, c}) == 3 and nv @ nv >= 1e-12:
            score[h] = int((((p64 - p64[a]) @ nv) ** 2 <= sc.THRESH ** 2 * (nv @ nv)).sum())
    assert r['info'][abi.RV_SEG_INFO_BEST_H] == int(np.argmax(score)) and score.max() == band.sum()
    assert (score == score.max()).sum() > 1, 'the case is meant to have a tie'
    # the plane row: the winner's normal and offset
    n, d = r['plane'][:3].astype(np.float64), float(r['plane'][3])
    assert np.abs((p64[band & (dist == 0)] @ n + d) / np.linalg.norm(n)).max() < 1e-5
    # the host mirror finds the same plane
    mask, plane, best_h = pcu.fit_table_plane(pts, seed=SEED, env_id=0)
    assert np.array_equal(mask, band) and best_h == r['info'][abi.RV_SEG_INFO_BEST_H] and np.array_equal(plane, r['plane'])
    assert len(pcu.remove_table(pts, seed=SEED)) == (~band).sum()


def test_plane_void_hypotheses_and_no_plane():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.001]], sh.F)
    p = sc.params(num_hypotheses=3, min_samples=1)
    # forced duplicates: only the last hypothesis is live
    for n in (3, 4):
        pl = sh.plane_stage(tri[:n], p, SEED, 0, ranks=np.array([[0, 0, 1], [1, 2, 2], [0, 1, 2]]))
        assert pl['scores'].tolist() == [-1, -1, n] and pl['best_h'] == 2
    # all void: duplicates, and three collinear points (|n|^2 < 1e-12)
    line = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], sh.F)
    for cloud, ranks in ((tri[:3], [[0, 0, 1], [1, 1, 1], [2, 1, 2]]), (line, [[0, 1, 2], [1, 2, 3], [0, 2, 3]])):
        pl = sh.plane_stage(cloud, p, SEED, 0, ranks=np.array(ranks))
        assert pl['best_h'] == -1 and not pl['mask'].any() and (pl['plane'] == 0).all()
    # keyed hypotheses on 3 and 4 points: void exactly where two ranks coincide
    for n in (3, 4):
        r = sh.segment(tri[:n], None, sc.params(num_hypotheses=64, min_samples=1), SEED, 5)
        o = sh.words(SEED, 5, 0, sh.hyp_ctr(np.arange(64)))
        rk = np.stack([sh.mulhi(o[k], n) for k in range(3)], axis=1)
        distinct = np.array([len(set(x)) == 3 for x in rk.tolist()])
        assert np.array_equal(r['scores'] >= 0, distinct) and 0 < distinct.sum() < 64
        assert r['info'][abi.RV_SEG_INFO_BEST_H] == int(np.flatnonzero(r['scores'] == r['scores'].max())[0])
    # n < 3 and T = 0: nothing removed, the flag says so
    for cloud, t in ((tri[:2], 50), (tri, 0)):
        r = sh.segment(cloud, None, sc.params(num_hypotheses=t, min_samples=1), SEED, 0)
        assert r['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_NO_PLANE and r['info'][abi.RV_SEG_INFO_PLANE] == 0
        assert r['info'][abi.RV_SEG_INFO_BEST_H] == -1 and (r['labels'] != sh.PLANE).all()


# ---- 3. grouping
def _rows(a):
    return {tuple(x) for x in np.asarray(a).tolist()}


@pytest.mark.parametrize('P', [1, 64, 65])
def test_grouping_contract(P):
    pts, lab = sc.grouping_cloud()
    sizes = np.bincount(lab)
    r = sh.segment(pts, None, sc.params(num_hypotheses=0, min_samples=5, num_clusters=8, num_points=P), SEED, 1)
    assert np.array_equal(r['labels'], lab) and r['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_FEWER
    assert r['slot_labels'].tolist() == [0, 1, 2, 3, 4, -1, -1, -1] and r['slot_counts'].tolist() == sizes.tolist() + [0, 0, 0]
    for s in range(8):
        cloud = r['clouds'][s]
        if s >= 5:
            assert (cloud == 0).all()
            continue
        members, m = _rows(pts[lab == s]), int(sizes[s])
        assert _rows(cloud) <= members
        if m >= P:
            assert len(_rows(cloud)) == P      # distinct members (all of them when m == P)
        if m == P:
            assert _rows(cloud) == members
    # more clusters than slots: the largest, ties to the smaller number; slots in ascending cluster number
    r2 = sh.segment(pts, None, sc.params(num_hypotheses=0, min_samples=5, num_clusters=2, num_points=P), SEED, 1)
    big = int(np.argmax(sizes))
    tie = int(np.flatnonzero(sizes == 64)[0])
    assert (sizes == 64).sum() == 2 and r2['slot_labels'].tolist() == sorted([big, tie]) and not r2['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_FEWER
    # another draw_index: other subsets, the same labels
    r3 = sh.segment(pts, None, sc.params(num_hypotheses=0, min_samples=5, num_clusters=8, num_points=P, draw_index=7), SEED, 1)
    assert np.array_equal(r3['labels'], r['labels']) and np.array_equal(r3['slot_counts'], r['slot_counts'])
    assert not np.array_equal(r3['clouds'], r['clouds'])


# ---- 4. the counter domains
def test_counter_words_never_meet_the_point_cloud_samplers():
    i = np.arange(65536, dtype=np.uint64)
    old = np.concatenate([f(b, i) for b in range(sh.RV_MAXB) for f in (sh.pc_key_ctr, sh.pc_draw_ctr)])
    assert len(old) == 2 * sh.RV_MAXB * 65536
    new = np.concatenate([sh.hyp_ctr(np.arange(abi.RV_SEG_MAX_HYPOTHESES)), sh.key_ctr(np.arange(0, 1 << 24, 255)), sh.key_ctr(i),
                          sh.key_ctr([(1 << 24) - 1])] + [sh.draw_ctr(s, i) for s in range(abi.RV_SEG_MAXSLOTS)])
    assert not np.intersect1d(old, new).size
    # the argument that covers every word: bit 31 clear and bits 28 .. 30 in {4, 5, 6}; the old words have bit 31 set or
    # nothing above bit 17
    assert (new >> np.uint64(31) == 0).all() and set(((new >> np.uint64(28)) & np.uint64(7)).tolist()) == {4, 5, 6}
    assert (((old >> np.uint64(31)) == 1) | ((old >> np.uint64(18)) == 0)).all()
    for k, ctr in ((4, sh.hyp_ctr(abi.RV_SEG_MAX_HYPOTHESES - 1)), (5, sh.key_ctr((1 << 24) - 1)),
                   (6, sh.draw_ctr(abi.RV_SEG_MAXSLOTS - 1, abi.RV_SEG_MAX_POINTS - 1))):
        assert int(ctr) >> 28 == k


# ---- 5. overflow
def test_overflow_keeps_evenly_spaced_points():
    pts = sc.overflow_cloud()
    assert len(pts) == 9000
    r = sh.segment(pts, None, sc.params(num_hypotheses=0), SEED, 2)
    slot = (np.arange(9000, dtype=np.int64) * sh.MAXPTS) // 9000
    first = np.concatenate([[True], slot[1:] != slot[:-1]])
    assert first.sum() == sh.MAXPTS and np.array_equal(r['kept'], np.flatnonzero(first))
    assert np.array_equal(r['labels'] == sh.SKIPPED, ~first)
    assert r['info'][abi.RV_SEG_INFO_SURVIVORS] == 9000 and r['info'][abi.RV_SEG_INFO_KEPT] == sh.MAXPTS
    assert r['info'][abi.RV_SEG_INFO_FLAGS] & sh.FLAG_OVERFLOW
    lab, _ = sh.dbscan(pts[first], sc.EPS, 50)      # min_samples is not rescaled
    assert np.array_equal(r['labels'][first], lab) and r['info'][abi.RV_SEG_INFO_CLUSTERS] == 3


# ---- 6. end to end on the float oracle's render
@pytest.fixture(scope='module')
def oracle_scene():
    from oracle import orc
    cfg, scene = sc.push_crop_cfg(sc.E2E_ENVS)
    ref = orc.OracleWorld(cfg, scene, double=False)
    ref.reset()
    cam = ref.camera()
    n_bodies = (ref.body_params()[:, :, 0] > 0).sum(axis=1)
    renders = [ref.render(e) for e in range(sc.E2E_ENVS)]
    return cfg, cam, n_bodies, renders


def test_deprojection_equals_the_camera_class(oracle_scene):
    import camera_host as ch
    cfg, cam, _, renders = oracle_scene
    depth, _ = renders[0]
    pts, valid = sh.deproject(depth, cam[0], (list(cfg.crop_min), list(cfg.crop_max)))
    want = ch.camera_of(cfg, cam[0]).deproject_depth_image(depth.astype(np.float64))
    want = np.asarray(want, np.float64).reshape(-1, 3)
    hit = depth.reshape(-1) > 0
    assert np.abs(pts[hit] - want[hit]).max() < 2e-6
    inside = ((want >= np.array(cfg.crop_min)) & (want <= np.array(cfg.crop_max))).all(axis=1)
    clear = np.abs(np.concatenate([want - np.array(cfg.crop_min), want - np.array(cfg.crop_max)], axis=1)).min(axis=1) > 1e-5
    assert np.array_equal(valid[clear] != 0, (hit & inside)[clear]) and (valid[~hit] == 0).all()


def test_clusters_of_the_oracle_render_are_the_bodies(oracle_scene):
    """Seed 3 of the push config: 8 of the 8 envs satisfy the precondition (bodies more than 2 eps apart, each with at
    least 2 min_samples points above the band); in each of them every kept cluster is pure and every body owns a slot."""
    cfg, cam, n_bodies, renders = oracle_scene
    qualifying = 0
    for e, (depth, seg) in enumerate(renders):
        pts, valid = sh.deproject(depth, cam[e], (list(cfg.crop_min), list(cfg.crop_max)))
        if not sc.precondition(pts, valid, seg, int(n_bodies[e])):
            continue
        qualifying += 1
        r = sh.segment(pts, valid, sc.params(), sc.world_seed(cfg), int(cfg.env_id_offset) + e)
        ok, why = sc.purity(r, seg, int(n_bodies[e]))
        assert ok, 'env %d: %s' % (e, why)
        assert not r['info'][abi.RV_SEG_INFO_FLAGS] & (sh.FLAG_NO_PLANE | sh.FLAG_BOUND)
    assert qualifying >= 3, qualifying


# ---- 7. bindings
def test_symbols_and_struct_layout(tmp_path):
    assert {'rv_deproject', 'rv_segment_cloud'} <= set(lib.SYMBOLS) and set(abi.SEGMENT_API) == {'rv_deproject', 'rv_segment_cloud'}
    src = tmp_path / 't.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rovat.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(rv_segment_params), '
                   'offsetof(rv_segment_params, draw_index), offsetof(rv_segment_params, num_points));return 0;}\n')
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 't')], check=True)
    out = subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(abi.rv_segment_params), abi.rv_segment_params.draw_index.offset,
                                     abi.rv_segment_params.num_points.offset]
    p = lib.segment_params(num_points=64, eps=0.03, draw_index=5)
    assert (p.num_hypotheses, p.min_samples, p.num_clusters, p.num_points, p.draw_index) == (50, 50, abi.RV_MAXB, 64, 5)
    assert abs(p.plane_thresh - 0.015) < 1e-9 and abs(p.eps - 0.03) < 1e-9
    with pytest.raises(TypeError):
        lib.segment_params(nope=1)
    handle = C.CDLL(lib.LIB_PATH) if os.path.exists(lib.LIB_PATH) else C.CDLL(lib.build())
    assert hasattr(handle, 'rv_deproject') and hasattr(handle, 'rv_segment_cloud')
