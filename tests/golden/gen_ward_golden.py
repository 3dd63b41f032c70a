"""Generate tests/golden/ward_golden.json: small jittered clouds labelled by scikit-learn's AgglomerativeClustering
itself (build container only; the tests need no scikit-learn).

    python tests/golden/gen_ward_golden.py

The call is the reference's second cluster() call: kneighbors_graph(n_neighbors=k, include_self=False), symmetrised, then
AgglomerativeClustering(linkage='ward', n_clusters=C, connectivity=...).  Every point lies on a 2^-20 m lattice inside a
0.5 m cube and is stored as its integer lattice coordinates, so that it is exact in float32.  A seed is taken only if the
restatement (tests/ward_host.py) keeps a relative gap of at least 1e-9 at every k-th neighbour, completion edge and merge
-- far above float64 rounding, so that scikit-learn's own arithmetic (its distances come from a dot-product expansion)
cannot choose differently -- and the test asserts the same again.  Only DATA is written: the points, k, C and
scikit-learn's labels.
"""
import json
import os
import sys
import warnings

import numpy as np
from sklearn.cluster import AgglomerativeClustering
from sklearn.neighbors import kneighbors_graph

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ward_host as wh  # noqa: E402

LATTICE = 1 << 20
MIN_GAP = 1e-9


def box(rng, lo, hi, m):
    return rng.uniform(lo, hi, (m, 3))


def three_boxes(rng):
    return np.concatenate([box(rng, (0.05, 0.05, 0.02), (0.11, 0.10, 0.07), 110), box(rng, (0.25, 0.08, 0.02), (0.30, 0.16, 0.06), 90),
                           box(rng, (0.12, 0.30, 0.02), (0.20, 0.36, 0.08), 100)]), 10, 3


def touching(rng, m):
    return np.concatenate([box(rng, (0.05, 0.05, 0.02), (0.11, 0.11, 0.07), m), box(rng, (0.11, 0.06, 0.02), (0.17, 0.12, 0.05), m),
                           box(rng, (0.30, 0.30, 0.02), (0.36, 0.36, 0.07), m)])


def blob(rng):
    return rng.normal((0.25, 0.25, 0.1), 0.04, (400, 3)), 30, 4


def clumps(rng):
    """five clumps 0.1 m apart with k = 4: the neighbour graph falls into at least five components"""
    return np.concatenate([rng.normal((0.08 + 0.09 * c, 0.1 + 0.07 * (c % 2), 0.05), 0.008, (40, 3)) for c in range(5)]), 4, 2


def complete(rng):
    return np.concatenate([rng.normal((0.1, 0.1, 0.05), 0.02, (40, 3)), rng.normal((0.2, 0.12, 0.05), 0.02, (35, 3)),
                           rng.normal((0.15, 0.25, 0.05), 0.02, (26, 3))]), 100, 3


def faces(rng):
    """what a depth camera keeps of four boxes: top faces and one side each, two of the boxes in contact"""
    parts = []
    for (x, y, s, h) in ((0.05, 0.05, 0.06, 0.05), (0.11, 0.05, 0.05, 0.03), (0.30, 0.10, 0.07, 0.06), (0.15, 0.32, 0.06, 0.04)):
        top = np.column_stack([rng.uniform(x, x + s, 80), rng.uniform(y, y + s, 80), np.full(80, h) + rng.normal(0, 0.0005, 80)])
        side = np.column_stack([rng.uniform(x, x + s, 32), np.full(32, y) + rng.normal(0, 0.0005, 32), rng.uniform(0.016, h, 32)])
        parts += [top, side]
    return np.concatenate(parts), 15, 4


def strip(rng):
    return np.column_stack([rng.uniform(0.02, 0.45, 250), rng.uniform(0.2, 0.23, 250), rng.uniform(0.02, 0.04, 250)]), 8, 5


CASES = [('three_boxes', three_boxes), ('touching_boxes', lambda r: (touching(r, 120), 20, 3)),
         ('touching_boxes_k100', lambda r: (touching(r, 140), 100, 3)), ('one_blob_cut_into_4', blob),
         ('disconnected_graph', clumps), ('complete_graph', complete), ('camera_faces', faces), ('strip', strip)]


def sklearn_labels(pts, k, C):
    conn = kneighbors_graph(pts, n_neighbors=min(k, len(pts) - 1), include_self=False)
    conn = 0.5 * (conn + conn.T)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # (the completion of a disconnected graph is announced as a warning)
        return AgglomerativeClustering(linkage='ward', n_clusters=C, connectivity=conn).fit(pts).labels_


def main():
    out = dict(lattice=LATTICE, min_gap=MIN_GAP, sklearn=__import__('sklearn').__version__, cases=[])
    for number, (name, make) in enumerate(CASES):
        for seed in range(50):
            rng = np.random.default_rng(1000 * number + seed)
            pts, k, C = make(rng)
            pts = pts[rng.permutation(len(pts))]
            lattice = np.clip(np.round(pts * LATTICE), 0, LATTICE // 2).astype(np.int64)
            p32 = lattice.astype(np.float32) / np.float32(LATTICE)
            r = wh.agglomerate(p32.astype(np.float64), k, C)
            if min(r['margins'].values()) >= MIN_GAP:
                break
        else:
            raise SystemExit('%s: no seed keeps the gaps' % name)
        assert 100 <= len(pts) <= 450 and 4 <= k <= 100, name
        labels = sklearn_labels(p32.astype(np.float64), k, C)
        assert wh.same_partition(labels, r['labels']), name
        out['cases'].append(dict(name=name, k=k, C=C, points=lattice.tolist(), labels=labels.tolist()))
        print('%-22s seed %d: %3d points, k %3d, C %d, %d components, gaps %s, sizes %s'
              % (name, seed, len(pts), k, C, r['components'], {a: '%.1e' % b for a, b in r['margins'].items()}, np.bincount(labels).tolist()))
    with open(os.path.join(HERE, 'ward_golden.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))


if __name__ == '__main__':
    main()
