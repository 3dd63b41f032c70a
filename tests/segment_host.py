"""NumPy restatement of csrc/rv_dev_segment.h (rv_deproject, rv_segment_cloud), for the tests: float32, operation for
operation, every product and sum rounded on its own; the counts are integers.  ``segment`` runs the three stages on one
env's cloud and returns what the kernel writes (labels, clouds, slots, plane, info) plus the intermediates the tests look
at.  The Philox block comes from tests/antipodal_host.py, as for the other ``*_host.py`` files."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

from antipodal_host import philox

F = np.float32
RV_STREAM_PC = 7            # (rv_dev_math.h; tests/test_segment_host.py checks it against the header)
RV_MAXB = 4
MAXPTS = 8192
HYP_CTR, KEY_CTR, DRAW_CTR = 0x40000000, 0x50000000, 0x60000000
INVALID, PLANE, SKIPPED = -3, -2, -4
FLAG_NO_PLANE, FLAG_OVERFLOW, FLAG_BOUND, FLAG_FEWER = 1, 2, 4, 8
FIELDS = ('num_hypotheses', 'plane_thresh', 'eps', 'min_samples', 'num_clusters', 'num_points', 'draw_index')


def pc_key_ctr(b, i):
    """RV_PC_KEY_CTR of rv_dev_obs.h"""
    return 0x80000000 | (np.asarray(b, np.uint64) << np.uint64(16)) | np.asarray(i, np.uint64)


def pc_draw_ctr(b, j):
    """RV_PC_DRAW_CTR of rv_dev_obs.h"""
    return (np.asarray(b, np.uint64) << np.uint64(16)) | np.asarray(j, np.uint64)


def hyp_ctr(h):
    return np.uint64(HYP_CTR) | np.asarray(h, np.uint64)


def key_ctr(i):
    return np.uint64(KEY_CTR) | np.asarray(i, np.uint64)


def draw_ctr(slot, j):
    return np.uint64(DRAW_CTR) | (np.asarray(slot, np.uint64) << np.uint64(16)) | np.asarray(j, np.uint64)


def fields(params):
    """params (a mapping or an rv_segment_params) -> dict of plain numbers"""
    get = (lambda k: params[k]) if isinstance(params, dict) else (lambda k: getattr(params, k))
    return {k: get(k) for k in FIELDS}


def words(seed, gid, draw, ctr):
    """the Philox block of counter words ctr (an array) for env gid -> four uint64 arrays"""
    ctr = np.atleast_1d(np.asarray(ctr, np.uint64))
    return philox(ctr, np.full_like(ctr, int(draw) & 0xFFFFFFFF), np.full_like(ctr, int(gid)), np.full_like(ctr, RV_STREAM_PC),
                  int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)


def mulhi(o, n):
    return (np.asarray(o, np.uint64) * np.uint64(n)) >> np.uint64(32)


def valid_mask(points, valid=None):
    p = np.asarray(points, F)
    with np.errstate(invalid='ignore'):
        ok = ((p - p) == F(0)).all(axis=1)
    if valid is not None:
        ok &= np.asarray(valid) != 0
    return ok


def hypothesis(pts, ranks):
    """(a, nv, nn) of the three valid-rank points: the base point, the unnormalised normal and its squared length"""
    a, b, c = pts[ranks[0]], pts[ranks[1]], pts[ranks[2]]
    u, v = b - a, c - a
    nv = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], F)
    nn = F(F(nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
    return a, nv, nn


def inliers(pts, a, nv, t2):
    d = (nv[0] * (pts[:, 0] - a[0]) + nv[1] * (pts[:, 1] - a[1])) + nv[2] * (pts[:, 2] - a[2])
    return d * d <= t2


def plane_stage(vp, p, seed, gid, ranks=None):
    """stage 1 on the valid points vp [n, 3] (float32, index order) -> dict(best_h, score, inlier mask, plane [4],
    scores [T] with -1 for void).  ranks [T, 3]: forced hypothesis ranks (the tests' void cases); None: the keyed ones."""
    n, T = len(vp), int(p['num_hypotheses'])
    out = dict(best_h=-1, score=0, mask=np.zeros(n, bool), plane=np.zeros(4, F), scores=np.full(T, -1, np.int64))
    if T == 0 or n < 3:
        return out
    if ranks is None:
        o = words(seed, gid, p['draw_index'], hyp_ctr(np.arange(T)))
        ranks = np.stack([mulhi(o[k], n) for k in range(3)], axis=1).astype(np.int64)
    thresh = F(p['plane_thresh'])
    best = None
    with np.errstate(over='ignore', invalid='ignore'):
        for h in range(T):
            r = ranks[h]
            if r[0] == r[1] or r[0] == r[2] or r[1] == r[2]:
                continue
            a, nv, nn = hypothesis(vp, r)
            if nn < F(1e-12):
                continue
            t2 = F(thresh * thresh) * nn
            m = inliers(vp, a, nv, t2)
            sc = int(m.sum())
            out['scores'][h] = sc
            if best is None or sc > best[0]:
                best = (sc, h, m, a, nv)
    if best is not None:
        sc, h, m, a, nv = best
        out.update(best_h=h, score=sc, mask=m,
                   plane=np.array([nv[0], nv[1], nv[2], -(F(nv[0] * a[0] + nv[1] * a[1]) + nv[2] * a[2])], F))
    return out


def thin(ns, cap=MAXPTS):
    """the survivor ranks that are kept: all of them, or with ns > cap the first of every slot floor(r * cap / ns)"""
    if ns <= cap:
        return np.arange(ns)
    r = np.arange(ns, dtype=np.int64)
    slot = (r * cap) // ns
    return np.flatnonzero(np.concatenate([[True], slot[1:] != slot[:-1]]))


def neighbours(pts, eps, block=512):
    """boolean [K, K]: ((dx dx + dy dy) + dz dz) <= eps * eps in float32"""
    pts = np.asarray(pts, F)
    K = len(pts)
    e2 = F(F(eps) * F(eps))
    out = np.zeros((K, K), bool)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, K, block):
            d = pts[s:s + block, None, :] - pts[None, :, :]
            out[s:s + block] = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= e2
    return out


def dbscan(pts, eps, min_samples):
    """stage 2 on the kept points [K, 3] -> labels int32 [K] (-1 noise) and the number of clusters"""
    K = len(pts)
    lab = np.full(K, -1, np.int32)
    if K == 0:
        return lab, 0
    nb = neighbours(pts, eps)
    core = nb.sum(axis=1) >= int(min_samples)
    ci = np.flatnonzero(core)
    # components of the core points; the root of a component = its smallest member
    root = np.full(K, K, np.int64)
    if len(ci):
        _, comp = connected_components(csr_matrix(nb[np.ix_(ci, ci)]), directed=False)
        first = np.full(comp.max() + 1, K, np.int64)
        np.minimum.at(first, comp, ci)
        root[ci] = first[comp]
    roots = np.unique(root[ci])
    number = {int(r): k for k, r in enumerate(roots)}
    for i in ci:
        lab[i] = number[int(root[i])]
    for i in np.flatnonzero(~core):
        rj = root[np.flatnonzero(nb[i] & core)]
        if len(rj):
            lab[i] = number[int(rj.min())]
    return lab, len(roots)


def group(pts, index, lab, ncl, p, seed, gid):
    """stage 3: kept points pts [K, 3] with their point indices and labels -> (clouds [C, P, 3], slot_labels [C],
    slot_counts [C], members: per slot the kept ranks that were emitted, in order)"""
    C, P = int(p['num_clusters']), int(p['num_points'])
    clouds = np.zeros((C, P, 3), F)
    sizes = np.bincount(lab[lab >= 0], minlength=ncl) if ncl else np.zeros(0, np.int64)
    order = sorted(range(ncl), key=lambda c: (-int(sizes[c]), c))[:C]
    chosen = sorted(order)
    slot_labels = np.full(C, -1, np.int32)
    slot_counts = np.zeros(C, np.int32)
    members = [np.zeros(0, np.int64) for _ in range(C)]
    for s, c in enumerate(chosen):
        mem = np.flatnonzero(lab == c)
        m = len(mem)
        slot_labels[s], slot_counts[s] = c, m
        if m >= P:
            key = words(seed, gid, p['draw_index'], key_ctr(index[mem]))[0]
            pick = mem[np.lexsort((np.arange(m), key))[:P]]
        else:
            pick = mem[mulhi(words(seed, gid, p['draw_index'], draw_ctr(s, np.arange(P)))[0], m).astype(np.int64)]
        clouds[s] = pts[pick]
        members[s] = pick
    return clouds, slot_labels, slot_counts, members


def segment(points, valid, params, seed, gid, ranks=None):
    """rv_segment_cloud on one env: points [M, 3], valid [M] or None, params (mapping or struct), the world's 64-bit seed,
    the global env id -> dict(labels [M], clouds, slot_labels, slot_counts, plane [4], info [8], kept: the point indices of
    the kept ranks, members: per slot the point indices emitted)"""
    p = fields(params)
    pts = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 3))
    M = len(pts)
    labels = np.full(M, INVALID, np.int32)
    ok = valid_mask(pts, valid)
    vi = np.flatnonzero(ok)
    pl = plane_stage(pts[vi], p, seed, gid, ranks)
    labels[vi[pl['mask']]] = PLANE
    si = vi[~pl['mask']]
    ns = len(si)
    keep = thin(ns)
    flags = (FLAG_NO_PLANE if pl['best_h'] < 0 else 0) | (FLAG_OVERFLOW if ns > MAXPTS else 0)
    labels[si] = SKIPPED
    ki = si[keep]
    lab, ncl = dbscan(pts[ki], p['eps'], p['min_samples'])
    labels[ki] = lab
    clouds, slot_labels, slot_counts, members = group(pts[ki], ki, lab, ncl, p, seed, gid)
    if ncl < int(p['num_clusters']):
        flags |= FLAG_FEWER
    info = np.array([len(vi), pl['score'], ns, len(ki), ncl, int((lab < 0).sum()), pl['best_h'], flags], np.int32)
    return dict(labels=labels, clouds=clouds, slot_labels=slot_labels, slot_counts=slot_counts, plane=pl['plane'], info=info,
                kept=ki, members=[ki[m] for m in members], scores=pl['scores'])


def segment_batch(points, valid, params, seed, gid0):
    """``segment`` for envs gid0, gid0 + 1, ... stacked as the kernel's buffers are"""
    res = [segment(points[e], None if valid is None else valid[e], params, seed, gid0 + e) for e in range(len(points))]
    return {k: np.stack([r[k] for r in res]) for k in ('labels', 'clouds', 'slot_labels', 'slot_counts', 'plane', 'info')}


def deproject(depth, cam_row, crop=None):
    """rv_deproject on one env: depth [H, W] float32, the env's calibration row [17] (rv_get_camera), crop = (min [3],
    max [3]) or None -> (points [H * W, 3] float32, valid uint8 [H * W]).  pixel_dir_cam, cam_position and deproject of
    rv_dev_obs.h."""
    d = np.asarray(depth, F)
    H, W = d.shape
    r = np.asarray(cam_row, F)
    fx, fy, cx, cy, sk = r[:5]
    R, t = r[5:14], r[14:17]
    v, u = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing='ij')
    y = (v - cy) / fy
    x = (u - cx - sk * y) / fx
    pcx, pcy, pcz = x * d, y * d, F(1.0) * d

    def tmulv(ax, ay, az):
        return (R[0] * ax + R[3] * ay + R[6] * az, R[1] * ax + R[4] * ay + R[7] * az, R[2] * ax + R[5] * ay + R[8] * az)
    o = tmulv(t[0], t[1], t[2])
    o = (-o[0], -o[1], -o[2])
    w = tmulv(pcx, pcy, pcz)
    pts = np.stack([o[0] + w[0], o[1] + w[1], o[2] + w[2]], axis=-1).astype(F).reshape(-1, 3)
    ok = (d > F(0)).reshape(-1)
    if crop is not None:
        lo, hi = np.asarray(crop[0], F), np.asarray(crop[1], F)
        ok &= (pts >= lo).all(axis=1) & (pts <= hi).all(axis=1)
    return pts, ok.astype(np.uint8)
