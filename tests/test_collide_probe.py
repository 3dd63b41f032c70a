"""The narrow phase of robovat_amd/csrc/rv_dev_collide.h, called directly (tests/probe/rv_collide_probe.hip compiled for
the host) and held to float64 references that call neither rv_dev_collide.h nor oracle/orc_collide.h.

* support_v: float64 argmax, first maximum on ties, wherever float32 rounding cannot change the winner.
* closest_segment / closest_triangle / simplex_weights: brute force over every sub-simplex (numpy.linalg.lstsq).
* gjk_epa: the result carries its own certificate.  Separated: the witnesses lie in their hulls (the half-spaces of
  scipy's ConvexHull; brute force over the sub-simplices for a point, a segment or a flat quad), so |pa - pb| is an
  UPPER bound of the distance; the support planes across the returned normal give a LOWER bound; `dist` must sit in
  that bracket and the bracket must be narrow.  (Not scipy.optimize.nnls for the flat hulls: on these inputs version 1.15
  returned points millimetres from the true projection with a reported residual of zero.)  Overlapping: the depth is the smallest facet offset of scipy's ConvexHull of the pairwise differences.
* simplex cache, lb_out, hit-or-miss at max_dist, man_add against a float64 model of the rule, plane_space.
* the host compile equals orc.eval_gjk(double=False) bit for bit (function level, outside any scene).

TOLERANCES.  Base: 2e-6 m in distance and 50 times that (1e-4) in normal and witnesses, as tests/test_independent_pin.py
holds the float oracle to on closed forms.  Where a class needs more, the FLOAT ORACLE's worst error against the same
certificate on the same pairs was measured (orc.eval_gjk(double=False), its own centroid guess) and four times that is
allowed -- never anything taken from the probe's output.  ORACLE_MEASURED below lists the measured figures (metres;
`bracket` is upper minus lower bound, `dist` is |dist - upper bound| or |depth - true depth|, `witness` the largest of
the hull-membership and pa - pb = dist n errors, `normal` the distance to the nearest facet normal attaining the depth);
test_tolerance_table_is_the_float_oracles_error recomputes them and fails if the table no longer says what the oracle
does.  allowed = max(base, 4 x measured):

  Above base (measured -> allowed, metres; everything not listed is below a quarter of its base and held to the base):
    random, separated        bracket 2.1e-06 -> 8.4e-06
    boxes, separated         dist 8.8e-07 -> 3.5e-06, bracket 8.7e-07 -> 3.5e-06     (the 0.65 m wall, the 0.61 m table slab)
    point, separated         bracket 3.2e-05 -> 1.3e-04     (a point against a segment or a quad: normal error times 3 cm)
    moved:boxes, separated   bracket 5.9e-07 -> 2.4e-06
    moved:parallel           bracket 9.3e-05 -> 3.7e-04     (faces turned <= 2 degrees that graze each other: the normal of a
                             micron-long v; an overlap below 0.1 mm can come back as a gap of microns)
    overlapping, `outside`   random 9.4e-03, boxes 8.0e-03, cylinders 8.1e-03, segment 9.2e-03, quad 1.1e-02, far 9.0e-03,
                             duplicates 9.5e-03, tiny 1.2e-04 -> four times each.  EPA keeps pa - pb = dist n and both
                             witnesses in the two support planes across n (`witness`, below 1.5e-07 in every class), but where
                             the triangle it ended on does not hold the foot of the perpendicular the witnesses lie IN those
                             planes up to a centimetre beside their hulls (rv_dev_collide.h, the end of epa()).
                             Four times a centimetre says little; the planes and pa - pb are what is held tightly.
  The far class (hulls 1.5 m from the origin, one float32 ulp there is 1.2e-7 m) stays inside the base: 1.6e-07 in dist.

EPA caps.  For nearly concentric 16-vertex round hulls (depth 4 to 6 cm) RV_EPA_MAX_VERTS / _FACES / _ITERS end the
expansion early: the reported depth is then too SMALL, never too large.  CONCENTRIC_SEED is chosen so that the float
oracle alone leaves out fewer than 5 % of the class: 6 of 256 pairs (2.3 %), short by 0.03 to 0.70 mm.  Over the seeds 1 to
12 the float oracle leaves out 6 to 19 of 256 (2.3 % to 7.4 %, by at most 1.1 mm) and is never too deep by more than 1.3e-8 m:
the 5 % cap holds for the seed, the one-sidedness for all of them.
"""
import itertools

import numpy as np
import pytest
from scipy.spatial import ConvexHull, QhullError

from oracle import orc
from probe import build as probe_build, collide_inputs as ci

F = np.float32
TOL_DIST, TOL_WIT = 2e-6, 1e-4
U32 = 2.0 ** -24                       # unit roundoff of float32

# the float oracle's worst figures per class (rounded up to two digits), see the module docstring
ORACLE_MEASURED = {
    ('random', False): dict(dist=1e-08, bracket=2.1e-06, normal=0, witness=4.5e-08, outside=0),
    ('random', True): dict(dist=7.1e-09, bracket=0, normal=3.6e-07, witness=1.4e-08, outside=0.0094),
    ('boxes', False): dict(dist=8.8e-07, bracket=8.7e-07, normal=0, witness=3.5e-06, outside=0),
    ('boxes', True): dict(dist=6.1e-08, bracket=0, normal=6.8e-07, witness=9e-08, outside=0.008),
    ('cylinders', False): dict(dist=6.4e-09, bracket=3.1e-08, normal=0, witness=5.7e-08, outside=0),
    ('cylinders', True): dict(dist=5.9e-09, bracket=0, normal=2.1e-07, witness=5e-09, outside=0.0081),
    ('point', False): dict(dist=6.1e-09, bracket=3.2e-05, normal=0, witness=1.1e-08, outside=0),
    ('point', True): dict(dist=4.4e-09, bracket=0, normal=2.1e-07, witness=1.1e-08, outside=4.4e-09),
    ('segment', False): dict(dist=5.3e-09, bracket=1.1e-07, normal=0, witness=1.8e-08, outside=0),
    ('segment', True): dict(dist=7.3e-09, bracket=0, normal=3.1e-07, witness=9.8e-09, outside=0.0092),
    ('quad', False): dict(dist=9.6e-09, bracket=1.7e-08, normal=0, witness=9.8e-08, outside=0),
    ('quad', True): dict(dist=7.5e-09, bracket=0, normal=2.1e-07, witness=6.9e-09, outside=0.011),
    ('far', False): dict(dist=1.6e-07, bracket=1.2e-07, normal=0, witness=2.5e-07, outside=0),
    ('far', True): dict(dist=7e-09, bracket=0, normal=1.2e-07, witness=1.4e-07, outside=0.009),
    ('tiny', False): dict(dist=4.2e-10, bracket=2.1e-09, normal=0, witness=5.8e-09, outside=0),
    ('tiny', True): dict(dist=2.6e-10, bracket=0, normal=2.6e-07, witness=2.8e-10, outside=0.00012),
    ('parallel', False): dict(dist=1.4e-08, bracket=1.9e-08, normal=0, witness=1.7e-08, outside=0),
    ('parallel', True): dict(dist=9.6e-09, bracket=0, normal=1.6e-07, witness=1.5e-08, outside=1.5e-08),
    ('duplicates', False): dict(dist=1.2e-08, bracket=3.5e-08, normal=0, witness=6.5e-08, outside=0),
    ('duplicates', True): dict(dist=9.2e-09, bracket=0, normal=3.5e-07, witness=1.4e-08, outside=0.0095),
    ('moved:random', False): dict(dist=7.6e-09, bracket=4.1e-08, normal=0, witness=6.3e-08, outside=0),
    ('moved:boxes', False): dict(dist=6e-08, bracket=5.9e-07, normal=0, witness=3.1e-06, outside=0),
    ('moved:cylinders', False): dict(dist=5.1e-09, bracket=1.6e-08, normal=1.2e-07, witness=3.3e-07, outside=0),
    ('moved:parallel', False): dict(dist=1.2e-08, bracket=9.3e-05, normal=1.2e-07, witness=1.5e-08, outside=5e-09),
}
CONCENTRIC_SEED = 10
CAP_SHARE = 0.05


def tol(cls, overlapping, key):
    base = TOL_DIST if key in ('dist', 'bracket') else TOL_WIT
    return max(base, 4.0 * ORACLE_MEASURED[(cls, overlapping)][key])


@pytest.fixture(scope='module')
def host():
    return probe_build.CollideProbe()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ support_v --
_SUPPORT = {}


def support_result(host):
    if not _SUPPORT:
        verts, cnt, dirs, _ = ci.support_cases()
        for k, v in zip(('proj', 'idx', 'v', 'proj2'), host.call('c_support_v', verts, cnt, dirs)):
            v.setflags(write=False)
            _SUPPORT[k] = v
    return _SUPPORT


def support_expectation():
    """(expected index or -1 where float32 rounding may decide, per item).
    The float32 projection is fl(fl(fl(x dx) + fl(y dy)) + fl(z dz)): three products and two sums, each with a
    relative error of at most u = 2^-24.  x dx and y dy pass through one product and two sums, z dz through one product
    and one sum: |error| <= ((1 + u)^3 - 1) (|x dx| + |y dy| + |z dz|) =: B(vertex).  B is zero where every product is
    an exact zero.  Two vertices whose float64 projections differ by more than the sum of their B cannot change order
    in float32; vertices that are bit-identical have bit-identical projections, and an exact computation (B = 0)
    reproduces float64 ties as ties.  In both cases the first index must win."""
    verts, cnt, dirs, _ = ci.support_cases()
    want = np.full(len(cnt), -1)
    for i in range(len(cnt)):
        V = verts[i].reshape(16, 3)[:cnt[i]].astype(np.float64)
        d = dirs[i].astype(np.float64)
        p = V @ d
        B = ((1 + U32) ** 3 - 1) * (np.abs(V) @ np.abs(d))
        first = int(np.argmax(p))                                   # numpy: the first maximum
        rivals = [j for j in range(cnt[i]) if p[first] - p[j] <= B[first] + B[j]]
        if all(np.array_equal(bits(verts[i].reshape(16, 3)[j]), bits(verts[i].reshape(16, 3)[rivals[0]])) for j in rivals) or \
                all(B[j] == 0.0 for j in rivals):
            want[i] = min(rivals)
    return want


def test_support_v_is_the_serial_first_maximum(host):
    verts, cnt, dirs, tags = ci.support_cases()
    got = support_result(host)
    want = support_expectation()
    decided = want >= 0
    # the generator must reach every case of the list, and rounding may leave only random hulls undecided
    for tag in ('max_first', 'max_last', 'tie', 'all_equal', 'dir_zero', 'signed_zero'):
        sel = np.array([t == tag for t in tags])
        assert sel.sum() >= 6 and decided[sel].all(), tag
    assert decided.mean() > 0.95
    assert set(cnt.tolist()) == {1, 2, 3, 8, 15, 16}
    last = np.array([t == 'max_last' for t in tags])
    assert (want[last] == cnt[last] - 1).all() and (want[np.array([t == 'max_first' for t in tags])] == 0).all()
    ties = np.array([t == 'tie' for t in tags])
    assert (want[ties] < cnt[ties] - 1).all()
    idx = got['idx'][:, 0]
    bad = np.nonzero(decided & (idx != want))[0]
    assert bad.size == 0, 'item %d (%s, n = %d): index %d, float64 first maximum %d' % (bad[0], tags[bad[0]], cnt[bad[0]], idx[bad[0]], want[bad[0]])
    # the vertex is the indexed one, bit for bit; the projection is its float32 dot product, in the header's order
    assert ((0 <= idx) & (idx < cnt)).all()
    V = verts.reshape(-1, 16, 3)[np.arange(len(cnt)), idx]
    assert np.array_equal(bits(got['v']), bits(V))
    pj = ((V[:, 0] * dirs[:, 0] + V[:, 1] * dirs[:, 1]).astype(F) + V[:, 2] * dirs[:, 2]).astype(F)
    assert np.array_equal(got['proj'][:, 0], pj)
    assert np.array_equal(got['proj2'][:, 0], got['proj'][:, 0])


# ---------------------------------------------------------------------------------------------- sub-simplex solvers --
def brute_force_closest(W):
    """The point of conv(W) closest to the origin, float64: for every non-empty sub-simplex the affine least-squares point,
    kept if all weights are non-negative; the nearest kept one.  -> (point, frozenset of the vertices that support it)"""
    W = np.asarray(W, np.float64)
    best = None
    for k in range(1, len(W) + 1):
        for sub in itertools.combinations(range(len(W)), k):
            w0 = W[sub[0]]
            if k == 1:
                lam = np.ones(1)
            else:
                E = (W[list(sub[1:])] - w0).T
                t = np.linalg.lstsq(E, -w0, rcond=None)[0]
                lam = np.concatenate([[1.0 - t.sum()], t])
            if (lam >= -1e-12).all():
                p = lam @ W[list(sub)]
                d = p @ p
                if best is None or d < best[0] - 1e-24:
                    best = (d, p, frozenset(s for s, l in zip(sub, lam) if l > 1e-9))
    return best[1], best[2]


def _check_closest(name, W, lam):
    """the closest POINT sum l_i w_i (weights are not unique on degenerate input), its distance, and the weights' form"""
    regions = {}
    for i in range(len(W)):
        want, region = brute_force_closest(W[i])
        regions[region] = regions.get(region, 0) + 1
        l = lam[i].astype(np.float64)
        assert (l >= 0).all() and abs(l.sum() - 1.0) < 1e-5, (name, i, l)
        got = l @ W[i].astype(np.float64)
        assert abs(np.linalg.norm(got) - np.linalg.norm(want)) < TOL_DIST, (name, i, got, want)
        assert np.linalg.norm(got - want) < TOL_WIT, (name, i, got, want)
    return regions


def test_closest_segment_against_brute_force(host):
    W = ci.simplex_cases(2)
    lam, = host.call('c_closest_segment', W.reshape(len(W), 6))
    regions = _check_closest('closest_segment', W, lam)
    assert all(regions.get(frozenset(r), 0) >= 20 for r in ((0,), (1,), (0, 1))), regions


def test_closest_triangle_hits_all_seven_regions(host):
    W = ci.simplex_cases(3)
    lam, = host.call('c_closest_triangle', W.reshape(len(W), 9))
    regions = _check_closest('closest_triangle', W, lam)
    want = [frozenset(c) for k in (1, 2, 3) for c in itertools.combinations(range(3), k)]
    assert len(want) == 7 and all(regions.get(r, 0) >= 20 for r in want), regions


def test_simplex_weights_hits_all_fifteen_regions(host):
    W = ci.simplex_cases(4)
    n = len(W)
    lam, flag = host.call('c_simplex_weights', W.reshape(n, 12), np.full(n, 4, np.int32))
    W64 = W.astype(np.float64)
    # signed distance of the origin to the four face planes, positive inside
    margin = np.full(n, np.inf)
    for i in range(n):
        for f in itertools.combinations(range(4), 3):
            o = [k for k in range(4) if k not in f][0]
            p, q, r = W64[i][list(f)]
            nrm = np.cross(q - p, r - p)
            ln = np.linalg.norm(nrm)
            if ln < 1e-12:
                margin[i] = 0.0
                continue
            nrm = nrm / ln * np.sign(nrm @ (W64[i][o] - p) or 1.0)
            margin[i] = min(margin[i], -(nrm @ p))
    inside, outside = margin > 1e-5, margin < -1e-5
    assert inside.sum() >= 30 and outside.sum() >= 400
    assert (flag[inside, 0] == 1).all() and (flag[outside, 0] == 0).all()
    sel = np.nonzero(flag[:, 0] == 0)[0]
    regions = _check_closest('simplex_weights', W[sel], lam[sel])
    want = [frozenset(c) for k in (1, 2, 3) for c in itertools.combinations(range(4), k)]
    assert len(want) == 14 and all(regions.get(r, 0) >= 15 for r in want), regions       # the fifteenth is `inside`
    # the lower simplices go through the same entry
    for nv in (1, 2, 3):
        Wn = np.zeros((len(ci.simplex_cases(max(nv, 2))), 4, 3), F)
        Wn[:, :max(nv, 2)] = ci.simplex_cases(max(nv, 2))
        lam, flag = host.call('c_simplex_weights', Wn.reshape(len(Wn), 12), np.full(len(Wn), nv, np.int32))
        assert (flag == 0).all() and (lam[:, nv:] == 0).all()
        _check_closest('simplex_weights n = %d' % nv, Wn[:, :nv], lam[:, :nv])


# ------------------------------------------------------------------------------------------------------------ gjk_epa --
def run_gjk(probe, pairs, **kw):
    hit, res, gc = probe.call('c_gjk_epa', *ci.gjk_arrays(pairs, **kw))
    return dict(hit=hit[:, 0], n=res[:, 0:3], dist=res[:, 3], pa=res[:, 4:7], pb=res[:, 7:10], lb=res[:, 10], gc=gc)


def run_oracle(pairs):
    """orc.eval_gjk(double=False) in the same layout (its guess is its own: the difference of the centroids)"""
    n = len(pairs)
    out = dict(hit=np.zeros(n, np.int32), n=np.zeros((n, 3), F), dist=np.zeros(n, F), pa=np.zeros((n, 3), F), pb=np.zeros((n, 3), F))
    for i, (A, B, _) in enumerate(pairs):
        r = orc.eval_gjk(A, B, double=False)
        if r is not None:
            out['hit'][i] = 1
            out['n'][i], out['dist'][i], out['pa'][i], out['pb'][i] = r['n'], r['dist'], r['pa'], r['pb']
    return out


_HULLS = {}


def distance_outside_hull(key, p, V):
    """How far p lies outside conv(V), float64.  A solid hull: the largest violation of the half-spaces of scipy's
    ConvexHull (cached per hull, never modified).  A flat or lower-dimensional one (a point, a segment, a quad): the
    distance to the nearest point of the hull, by brute force over its sub-simplices."""
    V = np.asarray(V, np.float64); p = np.asarray(p, np.float64)
    if key not in _HULLS:
        try:
            _HULLS[key] = ConvexHull(V).equations if len(V) >= 4 else None
        except QhullError:
            _HULLS[key] = None
    eq = _HULLS[key]
    if eq is not None:
        return max(0.0, float((eq[:, :3] @ p + eq[:, 3]).max()))
    assert len(V) <= 4, 'a flat hull of more than four vertices'
    q, _ = brute_force_closest(V - p)
    return float(np.linalg.norm(q))


_DIFF = {}


def difference_body(key, A, B):
    """ConvexHull of the <= 256 differences a - b, or None where it is flat; cached per pair (never modified)."""
    if key not in _DIFF:
        D = (A.astype(np.float64)[:, None, :] - B.astype(np.float64)[None, :, :]).reshape(-1, 3)
        try:
            _DIFF[key] = ConvexHull(D)
        except QhullError:
            _DIFF[key] = None
    return _DIFF[key]


def figures(key, pair, r, i):
    """The float64 certificate of result i: a dict of the figures the tolerances apply to, and what kind of result it is."""
    A, B, _ = pair
    n = r['n'][i].astype(np.float64); dist = float(r['dist'][i])
    pa, pb = r['pa'][i].astype(np.float64), r['pb'][i].astype(np.float64)
    da, db = distance_outside_hull(key + ('A',), pa, A), distance_outside_hull(key + ('B',), pb, B)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    nh = n / np.linalg.norm(n)
    out = dict(unit=abs(np.linalg.norm(n) - 1.0), witness=float(np.linalg.norm((pa - pb) - dist * n)), outside=max(da, db))
    out['pab'] = out['witness']
    hull = difference_body(key, A, B)
    signed = None if hull is None else float(hull.equations[:, 3].max())     # < 0: the origin is inside, depth = -signed
    out['true_signed'] = signed
    if dist >= 0.0:
        upper = float(np.linalg.norm(pa - pb))
        lower = float((A64 @ nh).min() - (B64 @ nh).max())
        out.update(kind='separated', upper=upper, lower=lower, bracket=upper - lower, dist=abs(dist - upper))
        out['witness'] = max(out['witness'], out['outside'])
    else:
        # EPA keeps pa - pb = dist n and puts the witnesses in the two support planes across n; where the triangle it ended
        # on does not hold the foot of the perpendicular they may lie beside their hulls IN those planes (rv_dev_collide.h,
        # the end of epa()): `outside` is measured apart from `witness`
        out['witness'] = max(out['witness'], abs(float(nh @ pa - (A64 @ nh).min())), abs(float(nh @ pb - (B64 @ nh).max())))
        out.update(kind='overlapping', dist=np.inf, normal=np.inf, too_deep=np.inf, depth=np.inf)
        if signed is not None:
            depth = -signed
            out['dist'] = abs(-dist - depth)
            out['too_deep'] = (-dist) - depth                # > 0: deeper than the truth
            off = -hull.equations[:, 3]
            # the outward normal of a facet that attains the reported depth (n points from B to A: -n is outward)
            near = np.abs(off - (-dist)) <= TOL_DIST + out['dist']
            out['normal'] = float(np.linalg.norm(hull.equations[near, :3] + n, axis=1).min())
            out['depth'] = depth
    return out


_FIG = {}


def class_figures(who, cls, overlapping, results):
    key = (who, cls, overlapping)
    if key not in _FIG:
        pairs = ci.gjk_pairs(cls, overlapping)
        _FIG[key] = [figures((cls, overlapping, i), pairs[i], results, i) if results['hit'][i] else None for i in range(len(pairs))]
    return _FIG[key]


def worst(figs, overlapping):
    """the worst figures of a class, as ORACLE_MEASURED lists them"""
    figs = [f for f in figs if f is not None]
    sep = [f for f in figs if f['kind'] == 'separated']
    ov = [f for f in figs if f['kind'] == 'overlapping']
    w = dict(unit=max(f['unit'] for f in figs), witness=max(f['witness'] for f in figs), dist=0.0, bracket=0.0, normal=0.0,
             outside=max([f['outside'] for f in ov] or [0.0]))
    if sep:
        w['dist'] = max(w['dist'], max(f['dist'] for f in sep)); w['bracket'] = max(f['bracket'] for f in sep)
    small = [f for f in ov if f['depth'] <= 0.02]
    if small:
        w['dist'] = max(w['dist'], max(f['dist'] for f in small)); w['normal'] = max(f['normal'] for f in small)
    return w


_RUN = {}


def probe_run(host, cls, overlapping):
    if (cls, overlapping) not in _RUN:
        _RUN[(cls, overlapping)] = run_gjk(host, ci.gjk_pairs(cls, overlapping))
    return _RUN[(cls, overlapping)]


CLASSES = [(c, o) for c in ci.GJK_CLASSES for o in (False, True)]
CACHE_CLASSES = ['random', 'boxes', 'cylinders', 'parallel']
MOVED = [('moved:' + c, False) for c in CACHE_CLASSES]


@pytest.mark.parametrize('cls,overlapping', CLASSES + MOVED)
def test_tolerance_table_is_the_float_oracles_error(cls, overlapping):
    """ORACLE_MEASURED is what the float oracle does on these pairs today: not smaller, and not rounded up by more than a
    quarter.  (Figures below a tenth of the base tolerance play no part and are only held below it.)"""
    w = worst(class_figures('oracle', cls, overlapping, run_oracle(ci.gjk_pairs(cls, overlapping))), overlapping)
    print('oracle', cls, overlapping, {k: '%.2e' % v for k, v in w.items()})
    rec = ORACLE_MEASURED[(cls, overlapping)]
    for key in ('dist', 'bracket', 'normal', 'witness', 'outside'):
        base = TOL_DIST if key in ('dist', 'bracket') else TOL_WIT
        assert w[key] <= 1.001 * rec[key], (key, w[key], rec[key])
        assert rec[key] <= max(1.25 * w[key], 0.1 * base), (key, w[key], rec[key])


@pytest.mark.parametrize('cls,overlapping', CLASSES)
def test_gjk_epa_certificate(host, cls, overlapping):
    pairs = ci.gjk_pairs(cls, overlapping)
    r = probe_run(host, cls, overlapping)
    assert r['hit'].all()                                             # max_dist = 1e9
    figs = class_figures('probe', cls, overlapping, r)
    kinds = [f['kind'] for f in figs]
    # the generator did its work: the class is (nearly) all of the kind asked for, by the REFERENCE's word
    truth_inside = np.array([f['true_signed'] is not None and f['true_signed'] < -TOL_DIST for f in figs])
    if overlapping:
        assert truth_inside.sum() >= 200, truth_inside.sum()
    else:
        assert (~truth_inside).all()
    w = worst(figs, overlapping)
    print('probe', cls, overlapping, {k: '%.2e' % v for k, v in w.items()})
    for i, f in enumerate(figs):
        ctx = (cls, overlapping, i, f)
        assert f['unit'] < 1e-5, ctx
        assert f['witness'] <= tol(cls, overlapping, 'witness'), ctx
        if truth_inside[i]:
            assert f['kind'] == 'overlapping', ctx
        if f['kind'] == 'separated':
            # upper and lower bound of the true distance bracket it, and dist with it
            assert f['bracket'] <= tol(cls, overlapping, 'bracket'), ctx
            assert f['dist'] <= tol(cls, overlapping, 'dist'), ctx
            # lb_out never exceeds the distance of two points of the hulls
            assert float(r['lb'][i]) <= f['upper'] + TOL_DIST, ctx
        else:
            assert f['true_signed'] is not None, ctx
            assert f['outside'] <= tol(cls, overlapping, 'outside'), ctx
            assert f['too_deep'] <= tol(cls, overlapping, 'dist'), ctx          # never deeper than the truth
            if f['depth'] <= 0.02:
                assert f['dist'] <= tol(cls, overlapping, 'dist'), ctx
                assert f['normal'] <= tol(cls, overlapping, 'normal'), ctx
            assert r['gc'][i, 0] == 0
    assert kinds.count('overlapping' if overlapping else 'separated') >= 200


@pytest.mark.parametrize('cls', ci.GJK_CLASSES)
def test_gjk_epa_hit_or_miss_at_max_dist_and_lb_out(host, cls):
    """A hit exactly when the distance is at most max_dist, a tolerance away from the boundary on either side; and a
    miss leaves an lb_out that is at most the true distance."""
    pairs = ci.gjk_pairs(cls, False)
    figs = class_figures('probe', cls, False, probe_run(host, cls, False))
    t = tol(cls, False, 'bracket') + tol(cls, False, 'dist')
    upper = np.array([f['upper'] for f in figs]); lower = np.array([f['lower'] for f in figs])
    assert (upper - lower <= tol(cls, False, 'bracket')).all()
    r = run_gjk(host, pairs, max_dist=(upper + t).astype(F))
    assert r['hit'].all()
    sel = np.nonzero(lower - t > 10 * t)[0]
    assert sel.size >= 100
    for md in (lower[sel] - t, 0.5 * lower[sel]):
        r = run_gjk(host, [pairs[i] for i in sel], max_dist=md.astype(F))
        assert not r['hit'].any()
        # the true distance, bracketed by the unconstrained call, exceeds max_dist; the bound of the miss does not exceed it
        assert (lower[sel] > md).all()
        assert (r['lb'] > 0).all() and (r['lb'] <= upper[sel] + TOL_DIST).all()


def test_nearly_concentric_round_hulls(host):
    """16-vertex cylinders and sphere samplings of 3 cm radius, centres <= 4 mm apart (depth mostly 3 to 6 cm).  The EPA caps may end
    the expansion early: an UNDERESTIMATE, never more, and in fewer than 5 % of the class.  CONCENTRIC_SEED is chosen so that the
    float oracle alone leaves out the share printed below, under the cap."""
    pairs = ci.concentric_pairs(CONCENTRIC_SEED)
    share = {}
    for who, r in (('oracle', run_oracle(pairs)), ('probe', run_gjk(host, pairs))):
        assert r['hit'].all() and (r['dist'] < 0).all() and np.median(r['dist']) < -0.04
        figs = [figures(('concentric', CONCENTRIC_SEED, i), pairs[i], r, i) for i in range(len(pairs))]
        assert max(f['too_deep'] for f in figs) <= TOL_DIST
        assert max(f['pab'] for f in figs) <= TOL_WIT              # pa - pb = dist n, also where the depth is cut short
        under = [f for f in figs if f['dist'] > TOL_DIST]
        share[who] = len(under) / float(len(pairs))
        print('%s: %d of %d underestimate the depth, by %.2e to %.2e m' % (who, len(under), len(pairs), min([f['dist'] for f in under] or [0]),
                                                                          max([f['dist'] for f in under] or [0])))
        for f in figs:
            if f['dist'] <= TOL_DIST:
                assert f['normal'] <= TOL_WIT and f['witness'] <= TOL_WIT
    assert share['oracle'] < CAP_SHARE and share['probe'] < CAP_SHARE, share


def mirror_pairs():
    """The inputs of test_independent_pin.test_gjk_epa_mirror_symmetric_overlaps with the guess orc_eval_gjk forms
    -> (pairs, [(A, B, signed distance)] of the first ones, the half extents of the concentric boxes, h)"""
    from test_independent_pin import _box, _rot
    h = 0.03
    A = _box([h, h, h])
    A2 = _box([h, h, h], R=_rot([0, 0, 1], np.pi / 4))
    cases = []
    for p_ in (0.004, 0.0006, 0.011):
        cases.append((A2, _box([h, h, h], [-(2.0 * np.sqrt(2.0) * h - p_), 0.0, 0.0], _rot([0, 1, 0], np.pi / 4)), -p_))
    for p_ in (0.003, 0.0004, 0.02):
        cases.append((A, _box([h, h, h], [-(2 * h - p_), 0.0, 0.0]), -p_))
    cases.append((A, _box([h, h, h], [-2 * h, 0.0, 0.0]), 0.0))
    boxes = ([0.01, 0.02, 0.015], [0.03, 0.03, 0.03], [0.05, 0.012, 0.04])
    th = np.arange(16) * 2 * np.pi / 16
    cyl = np.array([[0.02 * np.cos(a), 0.02 * np.sin(a), z] for z in (-0.01, 0.01) for a in th])
    extra = [(A, _box(hb)) for hb in boxes] + [(cyl[::2], _box([0.05, 0.05, 0.02]))]
    pairs = [(a.astype(F), b.astype(F), ci.oracle_guess(a, b)) for a, b in [c[:2] for c in cases] + extra]
    return pairs, cases, boxes, h


def test_touching_and_mirror_symmetric_cases_through_the_probe(host):
    """The inputs and expectations of test_independent_pin.test_gjk_epa_mirror_symmetric_overlaps (float tolerance)."""
    from test_independent_pin import _check
    t = 3e-6
    pairs, cases, boxes, h = mirror_pairs()
    r = run_gjk(host, pairs)
    assert r['hit'].all()
    res = [dict(n=r['n'][i].astype(np.float64), dist=float(r['dist'][i]), pa=r['pa'][i].astype(np.float64), pb=r['pb'][i].astype(np.float64))
           for i in range(len(pairs))]
    for i, (_, _, d) in enumerate(cases):
        _check(res[i], d, [1, 0, 0], t)
    for k, hb in enumerate(boxes):
        q = res[len(cases) + k]
        sums = np.array(hb) + h
        assert abs(-q['dist'] - sums.min()) < t, (q['dist'], sums)
        ax = int(np.argmin(sums)) if (np.sort(sums)[1] - sums.min()) > 1e-6 else int(np.argmax(np.abs(q['n'])))
        assert abs(abs(q['n'][ax]) - 1.0) < 50 * t and np.linalg.norm((q['pa'] - q['pb']) - q['dist'] * q['n']) < 50 * t
    q = res[-1]
    assert abs(-q['dist'] - 0.03) < t and abs(abs(q['n'][2]) - 1.0) < 50 * t


# ------------------------------------------------------------------------------------------------------ simplex cache --
def live_cache(gc):
    """a cache record without the words that mean nothing: the indices past its n, the pair of an empty one (a query leaves
    them as they were)"""
    gc = gc.copy()
    gc[gc[:, 0] == 0, 1] = 0
    gc[:, 2:][(np.arange(6)[None, :] % 3) >= gc[:, :1]] = 0
    return gc


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ('hit', 'n', 'dist', 'pa', 'pb', 'lb')) and \
        np.array_equal(live_cache(a['gc']), live_cache(b['gc']))


@pytest.mark.parametrize('cls', CACHE_CLASSES)
def test_simplex_cache(host, cls):
    pairs = ci.gjk_pairs(cls, False)
    n = len(pairs)
    first = run_gjk(host, pairs, use_gc=1, pair_id=5)
    uncached = probe_run(host, cls, False)
    assert first['hit'].all() and all(np.array_equal(bits(first[k]), bits(uncached[k])) for k in ('hit', 'n', 'dist', 'pa', 'pb', 'lb'))
    gc1 = first['gc']
    assert (gc1[:, 0] >= 1).all() and (gc1[:, 0] <= 3).all() and (gc1[:, 1] == 5).all()
    nA = np.array([len(p[0]) for p in pairs]); nB = np.array([len(p[1]) for p in pairs])
    for k in range(3):
        live = gc1[:, 0] > k
        assert (gc1[live, 2 + k] < nA[live]).all() and (gc1[live, 5 + k] < nB[live]).all() and (gc1[live, 2:] >= 0).all()
    moved = ci.gjk_pairs('moved:' + cls, False)
    mcls = 'moved:' + cls
    warm = run_gjk(host, moved, use_gc=1, pair_id=5, gc=gc1)
    cold = run_gjk(host, moved)
    empty = run_gjk(host, moved, use_gc=1, pair_id=5)
    assert warm['hit'].all() and cold['hit'].all()
    # an empty cache and no cache at all: the same query (the record left behind aside)
    assert all(np.array_equal(bits(cold[k]), bits(empty[k])) for k in ('hit', 'n', 'dist', 'pa', 'pb', 'lb'))
    # both pass the certificate and agree with each other
    sep = 0
    for i in range(n):
        fw = figures((mcls, False, i), moved[i], warm, i)
        fc = figures((mcls, False, i), moved[i], cold, i)
        for f in (fw, fc):
            assert f['witness'] <= tol(mcls, False, 'witness'), (i, f)
            if f['kind'] == 'separated':
                assert f['bracket'] <= tol(mcls, False, 'bracket') and f['dist'] <= tol(mcls, False, 'dist'), (i, f)
            else:
                assert f['too_deep'] <= tol(mcls, False, 'dist') and (f['depth'] > 0.02 or f['dist'] <= tol(mcls, False, 'dist')), (i, f)
        assert abs(float(warm['dist'][i]) - float(cold['dist'][i])) <= 2 * tol(mcls, False, 'dist') + tol(mcls, False, 'bracket'), (i, fw, fc)
        if fw['kind'] == fc['kind'] == 'separated':
            sep += 1
            # the closest feature is unique where the distance D is positive.  With a* - b* = D n* the closest pair, a unit n
            # whose support planes are `lower` apart has lower <= n . (a* - b*) = D n . n*, and D <= upper: so
            # |n - n*|^2 = 2 - 2 n . n* <= 2 (upper - lower) / D = 2 bracket / D, and the two normals differ by at most the sum
            d = max(fc['lower'], fw['lower'], 1e-9)
            bound = np.sqrt(2.0 * max(fw['bracket'], 0.0) / d) + np.sqrt(2.0 * max(fc['bracket'], 0.0) / d) + 1e-5
            assert np.linalg.norm(warm['n'][i].astype(np.float64) - cold['n'][i].astype(np.float64)) <= bound, (i, fw, fc, bound)
    assert sep >= 200
    # a cache of another pair, an empty one (n = 0 with stale indices), an index past either hull: as if there were none
    other = run_gjk(host, moved, use_gc=1, pair_id=6, gc=gc1)
    zero = gc1.copy(); zero[:, 0] = 0
    bad_a = gc1.copy(); bad_a[:, 2] = nA
    bad_b = gc1.copy(); bad_b[np.arange(n), 5 + gc1[:, 0] - 1] = nB + 3
    for name, q in (('pair', other), ('n = 0', run_gjk(host, moved, use_gc=1, pair_id=5, gc=zero)),
                    ('ia >= nA', run_gjk(host, moved, use_gc=1, pair_id=5, gc=bad_a)), ('ib >= nB', run_gjk(host, moved, use_gc=1, pair_id=5, gc=bad_b))):
        want = empty if name != 'pair' else run_gjk(host, moved, use_gc=1, pair_id=6)
        assert same_bits(q, want), name
    # ... and the cache is used where it is valid: some query ends on another simplex or in fewer steps
    assert not same_bits(warm, empty)


def test_cache_is_empty_after_a_hit_that_ended_in_epa(host):
    pairs = ci.gjk_pairs('random', True)
    stale = np.tile(np.array([[2, 9, 0, 1, 0, 0, 1, 0]], np.int32), (len(pairs), 1))
    r = run_gjk(host, pairs, use_gc=1, pair_id=9, gc=stale)
    deep = r['dist'] < 0
    assert deep.sum() >= 200 and (r['hit'] == 1).all()
    assert (r['gc'][deep, 0] == 0).all()


# ----------------------------------------------------------------------------------------- float oracle, function level --
@pytest.mark.parametrize('overlapping', [False, True])
def test_host_compile_equals_float_oracle_bit_for_bit(host, overlapping):
    """rv_dev_collide.h gjk_epa == orc_collide.h orc_gjk_epa (float) on the random class, with the guess orc_eval_gjk forms:
    hit, dist, n, pa, pb as words."""
    pairs = [(A, B, ci.oracle_guess(A, B)) for A, B, _ in ci.gjk_pairs('random', overlapping)]
    got, want = run_gjk(host, pairs), run_oracle(pairs)
    for k in ('hit', 'dist', 'n', 'pa', 'pb'):
        bad = np.nonzero((bits(got[k]).reshape(len(pairs), -1) != bits(want[k]).reshape(len(pairs), -1)).any(1))[0]
        assert bad.size == 0, (k, bad[:5], got[k][bad[:1]], want[k][bad[:1]])
    md = (0.5 * np.abs(want['dist'])).astype(F)
    if not overlapping:
        miss = run_gjk(host, pairs, max_dist=md)
        for i, (A, B, _) in enumerate(pairs[:64]):
            assert (orc.eval_gjk(A, B, max_dist=float(md[i]), double=False) is None) == (miss['hit'][i] == 0)


# ------------------------------------------------------------------------------------------------------------ man_add --
def area4(p0, p1, p2, p3):
    c = [np.cross(p0 - p1, p2 - p3), np.cross(p0 - p2, p1 - p3), np.cross(p0 - p3, p1 - p2)]
    return max(float(x @ x) for x in c)


def man_add_model(words, pt, col):
    """The rule in float64.  -> (slot written, new n, impulses kept?, outcome, smallest relative margin of a comparison)
    1. the same-collider point nearest within `breaking` is replaced and keeps its impulses;  2. otherwise append while
    n < 4;  3. otherwise keep the deepest and evict so that area4 is largest;  4. a new point's impulses are zero."""
    M = ci.MAN
    f = words.view(F).astype(np.float64); iw = words.view(np.int32)
    n = int(iw[M['n']])
    la = f[M['la']:M['la'] + 12].reshape(4, 3); dist = f[M['dist']:M['dist'] + 4]; cols = iw[M['col']:M['col'] + 4]
    p, pd, breaking = pt[0:3].astype(np.float64), float(pt[9]), float(pt[10])
    margin = np.inf
    cand = []
    for i in range(n):
        dd = float((la[i] - p) @ (la[i] - p))
        if cols[i] == col and breaking > 0.0:          # (breaking = 0: dd < 0 is false whatever the rounding)
            margin = min(margin, abs(dd - breaking ** 2) / breaking ** 2)
        if dd < breaking ** 2 and cols[i] == col:
            cand.append((dd, i))
    if cand:
        cand.sort()
        if len(cand) > 1:
            margin = min(margin, (cand[1][0] - cand[0][0]) / cand[1][0])
        return cand[0][1], n, True, 'replace', margin
    if n < 4:
        return n, n + 1, False, 'append', margin
    deepest = int(np.argmin(dist)) if dist.min() < pd else -1
    allv = np.sort(np.concatenate([dist, [pd]]))
    margin = min(margin, np.diff(allv).min() / 1e-3)
    r = [-1.0 if deepest == k else area4(p, *[la[j] for j in range(4) if j != k]) for k in range(4)]
    slot = int(np.argmax(r))
    rs = np.sort(r)
    margin = min(margin, (rs[-1] - rs[-2]) / rs[-1])
    return slot, 4, False, 'evict, deepest %d' % deepest, margin


def test_man_add_against_the_float64_model(host):
    mans, pts, cols, tags = ci.man_add_cases()
    assert host.man_words == ci.MAN['words'] == mans.shape[1]
    out, = host.call('c_man_add', mans, pts, cols)
    M = ci.MAN
    seen = {}
    for i in range(len(mans)):
        slot, n, keep, outcome, margin = man_add_model(mans[i], pts[i], cols[i])
        if margin < 1e-3:            # float32 and float64 might decide differently: not a case of this test
            seen['no margin'] = seen.get('no margin', 0) + 1
            continue
        seen[outcome] = seen.get(outcome, 0) + 1
        seen[tags[i] + ' -> ' + outcome.split(',')[0]] = seen.get(tags[i] + ' -> ' + outcome.split(',')[0], 0) + 1
        want = mans[i].copy()
        want.view(np.int32)[M['n']] = n
        want.view(np.int32)[M['col'] + slot] = cols[i]
        for name, src in (('la', pts[i, 0:3]), ('lb', pts[i, 3:6]), ('nrm', pts[i, 6:9])):
            want.view(F)[M[name] + 3 * slot:M[name] + 3 * slot + 3] = src
        want.view(F)[M['dist'] + slot] = pts[i, 9]
        if not keep:
            for name in ('ln', 'lt1', 'lt2'):
                want.view(F)[M[name] + slot] = 0.0
        diff = np.nonzero(out[i] != want)[0]
        assert diff.size == 0, (i, tags[i], outcome, 'words', diff, out[i][diff], want[diff])
    assert seen.get('no margin', 0) <= len(mans) // 20, seen
    for outcome in ('replace', 'append', 'evict, deepest -1', 'evict, deepest 0', 'evict, deepest 1', 'evict, deepest 2', 'evict, deepest 3'):
        assert seen.get(outcome, 0) >= 10, (outcome, seen)
    # a candidate within `breaking` of a point of ANOTHER collider replaces nothing; breaking = 0 replaces nothing at all
    assert seen.get('near_other -> replace', 0) == 0 and seen.get('near_other -> append', 0) + seen.get('near_other -> evict', 0) >= 30, seen
    assert seen.get('near_same -> replace', 0) >= 30, seen
    assert seen.get('breaking0 -> replace', 0) == 0 and seen.get('breaking0 -> append', 0) + seen.get('breaking0 -> evict', 0) >= 30, seen
    assert seen.get('deeper_than_all -> evict', 0) >= 30, seen


# -------------------------------------------------------------------------------------------------------- plane_space --
def test_plane_space_is_a_right_handed_frame(host):
    """Each component of t1, t2 goes through at most four float32 roundings (relative 2^-24 each) and the inputs are unit
    to one rounding per component: every identity below holds to 1e-6."""
    n = ci.plane_space_cases()
    z0 = F(0.70710678)
    assert (np.abs(n[:, 2]) == np.nextafter(z0, F(1))).sum() >= 2 and (np.abs(n[:, 2]) == z0).sum() >= 2
    assert (np.abs(n[:, 2]) == np.nextafter(z0, F(0))).sum() >= 2
    t, = host.call('c_plane_space', n)
    n64, t1, t2 = n.astype(np.float64), t[:, 0:3].astype(np.float64), t[:, 3:6].astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() < 2e-7
    e = 1e-6
    assert np.abs(np.linalg.norm(t1, axis=1) - 1).max() < e and np.abs(np.linalg.norm(t2, axis=1) - 1).max() < e
    assert np.abs((t1 * t2).sum(1)).max() < e and np.abs((t1 * n64).sum(1)).max() < e and np.abs((t2 * n64).sum(1)).max() < e
    assert np.abs(np.cross(t1, t2) - n64).max() < e


# ---------------------------------------------------------------------------------------------------- the probe itself --
def test_the_host_build_has_no_cross_lane_exports(host):
    """rv_dev_wave.h's primitives exist on the device only: the host library says so and computes nothing."""
    with pytest.raises(NotImplementedError):
        host.call('c_row_step', np.zeros((1, 64), np.uint32), sel=(0, 1))
    with pytest.raises(NotImplementedError):
        host.call('c_row_allreduce', np.zeros((1, 64), np.uint32), sel=(0,))


def test_the_baked_hash_covers_the_three_headers_and_the_probe(tmp_path, monkeypatch):
    """What the device library is checked against when it is loaded: a change of any of the four files changes it."""
    import shutil
    base = probe_build.collide_source_hash()
    files = probe_build.COLLIDE_HEADERS + (probe_build.COLLIDE_SRC,)
    assert [f.rsplit('/', 1)[1] for f in files] == ['rv_dev_math.h', 'rv_dev_wave.h', 'rv_dev_collide.h', 'rv_collide_probe.hip']
    seen = {base}
    for k in range(4):
        copies = []
        for j, f in enumerate(files):
            dst = tmp_path / ('%d_%d' % (k, j)) / f.rsplit('/', 1)[1]
            dst.parent.mkdir()
            shutil.copy(f, dst)
            if j == k:
                with open(dst, 'a') as fh:
                    fh.write('\n// touched\n')
            copies.append(str(dst))
        monkeypatch.setattr(probe_build, 'COLLIDE_HEADERS', tuple(copies[:3]))
        monkeypatch.setattr(probe_build, 'COLLIDE_SRC', copies[3])
        seen.add(probe_build.collide_source_hash())
    assert len(seen) == 5
