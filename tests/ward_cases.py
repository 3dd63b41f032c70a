"""The clouds that tests/test_ward_host.py and tests/test_gpu_ward.py share: the golden clouds that scikit-learn's
AgglomerativeClustering labelled (tests/golden/ward_golden.json), the tie lattice, the boundary sizes, the overflow and
grouping clouds, and the push scene with two bodies in contact."""
import json
import os

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
MIN_GAP = 1e-9            # the relative gap every golden cloud keeps at the k-th neighbour, at a completion edge, at a merge


def params(**kw):
    p = dict(num_neighbors=100, num_groups=4, num_points=256, draw_index=0)
    p.update(kw)
    return p


def golden():
    """[dict(name, points float32 [n, 3], k, C, labels: scikit-learn's)], the file's header"""
    with open(os.path.join(HERE, 'golden', 'ward_golden.json')) as f:
        g = json.load(f)
    out = []
    for c in g['cases']:
        lattice = np.array(c['points'], np.int64)
        out.append(dict(name=c['name'], points=(lattice.astype(F) / F(g['lattice'])), k=int(c['k']), C=int(c['C']),
                        labels=np.array(c['labels'], np.int64)))
    return out, g


def tie_lattice():
    """125 points of a 5 x 5 x 5 lattice (1/64 m: every distance and every early w is exact and many are equal), 40 of
    them a second time, shuffled: equal distances at the k-th neighbour, equal w at the merges, w = 0 between duplicates"""
    rng = np.random.default_rng(31)
    g = np.arange(5)
    pts = np.array([[a, b, c] for a in g for b in g for c in g], np.int64)
    pts = np.concatenate([pts, pts[rng.choice(len(pts), 40, replace=False)]])
    return (pts[rng.permutation(len(pts))].astype(F) / F(64))


def sized_cloud(n, seed=0):
    """n points in three blobs of unequal size"""
    rng = np.random.default_rng(100 + seed)
    centers = np.array([(0.2, 0.2, 0.05), (0.32, 0.22, 0.05), (0.25, 0.45, 0.08)])
    which = rng.integers(0, 3, n)
    return (centers[which] + rng.normal(0.0, 0.025, (n, 3))).astype(F)


def overflow_cloud(n=2500):
    """n points in four flat patches (more than RV_WARD_MAXPTS = 2048)"""
    rng = np.random.default_rng(41)
    centers = np.array([(0.2, 0.2, 0.05), (0.5, 0.2, 0.05), (0.2, 0.5, 0.05), (0.5, 0.5, 0.08)])
    which = rng.integers(0, 4, n)
    return (centers[which] + rng.uniform(-0.06, 0.06, (n, 3)) * [1.0, 1.0, 0.1]).astype(F)


GROUP_SIZES = (64, 100, 30, 65)


def grouping_cloud():
    """four tight blobs of GROUP_SIZES members far apart, interleaved in index order so that blob g is the one whose
    first member has the g-th smallest index -> (points float32 [M, 3], blob of every point).  Any sensible clustering
    into four groups returns the blobs."""
    rng = np.random.default_rng(42)
    pts = np.concatenate([np.array([0.1 + 0.2 * g, 0.3, 0.05]) + rng.uniform(-0.01, 0.01, (m, 3)) for g, m in enumerate(GROUP_SIZES)])
    lab = np.concatenate([np.full(m, g) for g, m in enumerate(GROUP_SIZES)])
    order = rng.permutation(len(pts))
    first = [int(np.flatnonzero(lab[order] == g)[0]) for g in range(len(GROUP_SIZES))]
    rename = np.argsort(np.argsort(first))
    return pts[order].astype(F), rename[lab[order]]


def mixed_cloud():
    """a cloud as rv_segment_cloud leaves it: 300 clustered points among noise, plane, invalid and skipped ones, and two
    clustered points with a non-finite coordinate -> (points [M, 3], labels [M])"""
    rng = np.random.default_rng(43)
    pts = sized_cloud(400, 7)
    lab = np.zeros(400, np.int32)
    lab[rng.choice(400, 100, replace=False)] = rng.choice([-1, -2, -3, -4], 100)
    lab[lab >= 0] = rng.integers(0, 3, int((lab >= 0).sum()))
    pos = np.flatnonzero(lab >= 0)
    pts[pos[3], 1] = np.nan
    pts[pos[17], 2] = np.inf
    pts[np.flatnonzero(lab == -3)[:5]] = np.nan
    return pts, lab


CONTACT_OFFSET = (0.0, 0.06)      # body 1 this far (x, y) from body 0 of seed 3's env 0: DBSCAN joins the two


def contact_world(n_envs=1):
    """the float oracle's push world of tests/segment_cases.py, reset -> (cfg, scene, oracle world)"""
    import segment_cases as sc
    from oracle import orc
    cfg, scene = sc.push_crop_cfg(n_envs)
    ref = orc.OracleWorld(cfg, scene, double=False)
    ref.reset()
    return cfg, scene, ref


def place_in_contact(state, offset):
    """body 1 at body 0's pose shifted by `offset` (x, y), at rest: a copy of the [N, B, 13] state"""
    s = np.array(state, np.float64)
    s[:, 1, :] = s[:, 0, :]
    s[:, 1, 0] += offset[0]
    s[:, 1, 1] += offset[1]
    s[:, :2, 7:] = 0.0
    return s
