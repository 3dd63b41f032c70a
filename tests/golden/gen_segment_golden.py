"""Generate tests/golden/segment_golden.json: small clouds labelled by scikit-learn's DBSCAN itself (build container
only; the tests need no scikit-learn).

    python tests/golden/gen_segment_golden.py

Every point lies on a 1/1024 m lattice inside a 0.3 m cube and is stored as its integer lattice coordinates, so that a
squared distance is exact in float32 and in float64 alike.  With eps = 0.02 the threshold eps^2 * 1024^2 = 419.43 lies
between the integers 419 and 420: no pair is within 4e-7 m^2 of eps^2 (asserted here and again in the test).  Only DATA is
written: the points, the mask, the parameters and scikit-learn's labels of the valid points.
"""
import json
import os

import numpy as np
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 0.02
LATTICE = 1024
MARGIN = 4e-7


def grid(center, half=1, step=4):
    r = np.arange(-half, half + 1) * step
    return np.array([[center[0] + a, center[1] + b, center[2] + c] for a in r for b in r for c in r], np.int64)


def two_blobs_border():
    """a border point (index 0) next to core points of both blobs: the blob that comes first in index order is cluster 0
    and wins; a second border point closes the array"""
    right, left = grid((94, 50, 50)), grid((50, 50, 50))
    return np.concatenate([[[72, 50, 50]], right, left, [[72, 50, 54]]]), None, 27


def chain():
    """200 points 15 lattice units apart along a path that snakes through the cube, rows 30 units apart: one component
    199 hops long, index 0 at one end"""
    pts, x, y, d = [], 5, 5, 1
    while len(pts) < 200:
        for _ in range(20):
            pts.append((x, y, 150)); x += 15 * d
        x -= 15 * d
        pts.append((x, y + 15, 150))
        y += 30; d = -d
    return np.array(pts[:200], np.int64), None, 2


def all_noise():
    r = np.arange(4) * 40 + 10
    return np.array([[a, b, c] for a in r for b in r for c in r], np.int64), None, 2


def exact_min_samples():
    """a blob of exactly min_samples points (all core) and one of min_samples - 1 (all noise)"""
    a = grid((60, 60, 60))[:10]
    b = grid((200, 200, 200))[:9]
    return np.concatenate([a, b]), None, 10


def duplicates():
    rng = np.random.default_rng(3)
    blob = np.concatenate([np.repeat([[100, 100, 100]], 30, axis=0), np.repeat([[250, 40, 40]], 5, axis=0),
                           grid((104, 100, 100), 1, 3), grid((104, 100, 100), 1, 3)[:7]])
    return blob[rng.permutation(len(blob))], None, 6


def masked_bridge():
    """384 points, 383 valid: the masked one would be a core point that joins the two blobs"""
    rng = np.random.default_rng(4)
    a, b = grid((50, 50, 50)), grid((94, 50, 50))
    rest = rng.integers(130, 300, (384 - 55, 3))      # (clear of the blobs; some of it dense enough to cluster)
    pts = np.concatenate([a, [[72, 50, 50]], b, rest])
    valid = np.ones(len(pts), np.uint8)
    valid[27] = 0
    return pts, valid, 10


def too_few():
    return grid((150, 150, 150))[:20], None, 50


def overlapping(seed, n_blobs, ms):
    rng = np.random.default_rng(seed)
    parts = [np.round(rng.normal(rng.uniform(60, 240, 3), rng.uniform(6, 14), (int(rng.integers(40, 110)), 3))) for _ in range(n_blobs)]
    parts.append(rng.integers(0, 300, (40, 3)))
    pts = np.clip(np.concatenate(parts), 0, 307).astype(np.int64)[:400]
    return pts[rng.permutation(len(pts))], None, ms


CASES = [('two_blobs_border', two_blobs_border), ('chain', chain), ('all_noise', all_noise),
         ('exact_min_samples', exact_min_samples), ('duplicates', duplicates), ('masked_bridge', masked_bridge),
         ('too_few', too_few), ('overlapping_a', lambda: overlapping(11, 3, 8)), ('overlapping_b', lambda: overlapping(12, 4, 12))]


def margin_ok(pts):
    d = pts[:, None, :] - pts[None, :, :]
    d2 = (d * d).sum(-1).astype(np.float64) / (LATTICE * LATTICE)
    return float(np.abs(d2 - EPS * EPS).min()) > MARGIN


def main():
    out = dict(eps=EPS, lattice=LATTICE, margin=MARGIN, sklearn=__import__('sklearn').__version__, cases=[])
    for name, make in CASES:
        pts, valid, ms = make()
        assert len(pts) <= 400 and pts.min() >= 0 and pts.max() <= 307, name
        assert margin_ok(pts), name
        ok = np.ones(len(pts), bool) if valid is None else valid != 0
        labels = DBSCAN(eps=EPS, min_samples=ms).fit(pts[ok].astype(np.float64) / LATTICE).labels_
        out['cases'].append(dict(name=name, min_samples=ms, points=pts.tolist(), valid=None if valid is None else valid.tolist(),
                                 labels=labels.tolist()))
        print('%-20s %4d points, %d clusters, %d noise' % (name, len(pts), labels.max() + 1, int((labels < 0).sum())))
    with open(os.path.join(HERE, 'segment_golden.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))


if __name__ == '__main__':
    main()
