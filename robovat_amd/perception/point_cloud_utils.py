"""Segmentation-id conversion and per-body grouping of a point cloud, with the
behaviour of ``robovat/perception/point_cloud_utils.py:23-39,110-157`` (pinned by
``tests/golden/camera_golden.json``: shapes, zero fill, with-replacement rule)."""
import numpy as np


def downsample(point_cloud, num_samples):
    """``num_samples`` points drawn from the cloud: without replacement when it has
    enough points, with replacement otherwise."""
    n = point_cloud.shape[0]
    inds = np.random.choice(np.arange(n), size=num_samples, replace=n < num_samples)
    return point_cloud[inds]


def convert_segment_ids(segmask, body_ids):
    """Body uids in a segmentation mask -> their index in ``body_ids``; -1 elsewhere."""
    segmask = np.asarray(segmask)
    out = np.full_like(segmask, -1)
    for i, uid in enumerate(body_ids):
        out[segmask == uid] = i
    return out


def group_by_labels(point_cloud, segmask, num_clusters, num_samples):
    """[num_clusters, num_samples, 3] float32: per label a downsampled copy of its points,
    zeros for labels without points."""
    out = np.zeros([num_clusters, num_samples, 3], dtype=np.float32)
    for i in range(num_clusters):
        inds = np.where(segmask == i)[0]
        if len(inds) > 0:
            out[i] = downsample(point_cloud[inds], num_samples)
    return out


# ---- the real-sensor branch (point_cloud_utils.py:42-108, 160-190): host mirrors of rv_segment_cloud's stages
# (csrc/rv_dev_segment.h).  NumPy, float32 tests as on the device; the batched versions are
# ``lib.World.segment_cloud`` / ``VecPushEnv.clustered_point_cloud``.

def segment_by_ids(point_cloud, segmask, body_ids, num_samples):
    """[num_bodies, num_samples, 3] float32: per body id a downsampled copy of the points that carry it, zeros for a
    body without points."""
    out = np.zeros([len(body_ids), num_samples, 3], dtype=np.float32)
    segmask = np.asarray(segmask)
    for i, uid in enumerate(body_ids):
        inds = np.where(segmask == uid)[0]
        if len(inds) > 0:
            out[i] = downsample(point_cloud[inds], num_samples)
    return out


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/rv_dev_math.h) over uint64 arrays holding 32-bit words"""
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = [np.asarray(x, np.uint64) & m32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & m32, np.uint64(k1) & m32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0, c1, c2, c3


def fit_table_plane(point_cloud, thresh=0.015, num_hypotheses=50, seed=0, env_id=0, draw_index=0):
    """The plane stage of ``rv_segment_cloud`` on one cloud [n, 3] (all points taken as valid): hypothesis h takes the
    points of ranks mulhi(o_k, n) of the Philox block (0x40000000 | h, draw_index, env_id, RV_STREAM_PC; seed), is void when
    two ranks coincide or |(b - a) x (c - a)|^2 < 1e-12, and scores the points with (nv . (p - a))^2 <= thresh^2 |nv|^2;
    the largest score wins, ties to the smallest h.  Returns (inlier mask [n], plane [4] = (nv, -nv . a), best h or -1)."""
    f = np.float32
    p = np.asarray(point_cloud, f).reshape(-1, 3)
    n, t = len(p), int(num_hypotheses)
    mask, plane, best_h, best = np.zeros(n, bool), np.zeros(4, f), -1, -1
    if t == 0 or n < 3:
        return mask, plane, best_h
    ctr = np.uint64(0x40000000) | np.arange(t, dtype=np.uint64)
    o = _philox(ctr, np.full_like(ctr, int(draw_index)), np.full_like(ctr, int(env_id)), np.full_like(ctr, 7),
                int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    ranks = np.stack([(o[k] * np.uint64(n)) >> np.uint64(32) for k in range(3)], axis=1).astype(np.int64)
    th = f(thresh)
    with np.errstate(over='ignore', invalid='ignore'):
        for h in range(t):
            r0, r1, r2 = ranks[h]
            if r0 == r1 or r0 == r2 or r1 == r2:
                continue
            a, u, v = p[r0], p[r1] - p[r0], p[r2] - p[r0]
            nv = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], f)
            nn = f(f(nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
            if nn < f(1e-12):
                continue
            d = (nv[0] * (p[:, 0] - a[0]) + nv[1] * (p[:, 1] - a[1])) + nv[2] * (p[:, 2] - a[2])
            m = d * d <= f(th * th) * nn
            if int(m.sum()) > best:
                best, best_h, mask = int(m.sum()), h, m
                plane = np.array([nv[0], nv[1], nv[2], -(f(nv[0] * a[0] + nv[1] * a[1]) + nv[2] * a[2])], f)
    return mask, plane, best_h


def remove_table(point_cloud, thresh=0.015, num_hypotheses=50, seed=0, env_id=0, draw_index=0):
    """The cloud without the points within ``thresh`` of the fitted table plane (``fit_table_plane``).  The reference fits
    with PCL's RANSAC; here the hypotheses are Philox-keyed, as on the device, so that the result is reproducible."""
    mask, _, _ = fit_table_plane(point_cloud, thresh, num_hypotheses, seed, env_id, draw_index)
    return np.asarray(point_cloud)[~mask]


def dbscan_labels(point_cloud, eps=0.02, min_samples=50):
    """DBSCAN as ``rv_segment_cloud`` defines it, equal to scikit-learn's labelling: j neighbours i iff the float32
    squared distance (dx dx + dy dy) + dz dz <= eps * eps; core = at least ``min_samples`` neighbours, itself included;
    clusters = the components of the core points, numbered by ascending smallest member; a non-core point next to a core
    point takes the smallest cluster number among its core neighbours; the rest is -1."""
    f = np.float32
    p = np.asarray(point_cloud, f).reshape(-1, 3)
    n = len(p)
    lab = np.full(n, -1, np.int64)
    e2 = f(f(eps) * f(eps))
    rows = []
    for s in range(0, n, 512):
        d = p[s:s + 512, None, :] - p[None, :, :]
        rows.append(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) <= e2)
    nb = np.concatenate(rows) if rows else np.zeros((0, 0), bool)
    core = nb.sum(axis=1) >= int(min_samples)
    k = 0
    for i in np.flatnonzero(core):      # (ascending: a new component starts at its smallest member)
        if lab[i] >= 0:
            continue
        lab[i] = k
        todo = [i]
        while todo:
            j = todo.pop()
            new = np.flatnonzero(nb[j] & core & (lab < 0))
            lab[new] = k
            todo.extend(new.tolist())
        k += 1
    for i in np.flatnonzero(~core):
        c = lab[np.flatnonzero(nb[i] & core)]
        if len(c):
            lab[i] = c.min()
    return lab


def cluster(point_cloud, num_clusters, method='agg'):
    """Integer labels [n].  'dbscan': ``dbscan_labels`` with the reference's eps 0.02 and min_samples 50 (-1 = noise;
    ``num_clusters`` is not used, as in the reference).  'agg': Ward agglomeration on the symmetrised 100-nearest-neighbour
    graph into exactly ``num_clusters`` groups, through scikit-learn -- not built on the device."""
    if method == 'dbscan':
        return dbscan_labels(point_cloud, eps=0.02, min_samples=50)
    if method == 'agg':
        try:
            from sklearn.neighbors import kneighbors_graph
            from sklearn.cluster import AgglomerativeClustering
        except ImportError:
            raise RuntimeError("cluster(method='agg') needs scikit-learn, which is not installed; "
                               "method='dbscan' needs NumPy only")
        pts = np.asarray(point_cloud)
        conn = kneighbors_graph(pts, n_neighbors=min(100, len(pts) - 1), include_self=False)
        conn = 0.5 * (conn + conn.T)
        return AgglomerativeClustering(linkage='ward', n_clusters=num_clusters, connectivity=conn).fit(pts).labels_.astype(np.int64)
    raise ValueError('Unrecognized method: %r.' % (method,))


# ---- the second cluster() call of that branch: the definition of rv_ward_groups' clustering (csrc/rv_dev_ward.h,
# DESIGN.md §26) in NumPy, float64, without scikit-learn; the batched version is ``lib.World.ward_groups``.

def _ward_dist(mean, cnt, a, b):
    """compute_ward_dist of scikit-learn between cluster a and the clusters b (an index array)"""
    nn = (cnt[a] * cnt[b]) / (cnt[a] + cnt[b])
    t = mean[a][None, :] - mean[b]
    return ((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]) * nn


def ward_graph(points, n_neighbors=100):
    """The connectivity of ``ward_labels``: (adjacency bool [n, n], squared distances float64 [n, n], number of components
    before completion).  Point i is joined to its min(k, n - 1) nearest points, smallest (d2, j) first, the graph is
    symmetrised, and for every pair of components a > b (numbered by smallest member) the pair (p in a, q in b) smallest in
    (d2, p, q) is joined too (scikit-learn's ``_fix_connected_components``)."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    dx, dy, dz = [p[:, None, c] - p[None, :, c] for c in range(3)]
    d2 = (dx * dx + dy * dy) + dz * dz
    adj = np.zeros((n, n), bool)
    keff = min(int(n_neighbors), n - 1)
    if keff > 0:
        dd = d2.copy()
        np.fill_diagonal(dd, np.inf)
        near = np.argsort(dd, axis=1, kind='stable')[:, :keff]
        adj[np.arange(n)[:, None], near] = True
        adj |= adj.T
    comp = np.full(n, -1, np.int64)
    ncomp = 0
    for i in range(n):      # (ascending: a new component starts at its smallest member)
        if comp[i] >= 0:
            continue
        comp[i] = ncomp
        front = np.array([i])
        while len(front):
            new = np.flatnonzero(adj[front].any(axis=0) & (comp < 0))
            comp[new] = ncomp
            front = new
        ncomp += 1
    members = [np.flatnonzero(comp == c) for c in range(ncomp)]
    for a in range(ncomp):
        for b in range(a):
            block = d2[np.ix_(members[a], members[b])]
            ia, ib = np.unravel_index(np.argmin(block), block.shape)      # (the first minimum in row-major order)
            adj[members[a][ia], members[b][ib]] = adj[members[b][ib], members[a][ia]] = True
    return adj, d2, ncomp


def ward_labels(point_cloud, num_clusters, n_neighbors=100):
    """Integer labels [n]: Ward agglomeration on the symmetrised ``n_neighbors``-nearest-neighbour graph into exactly
    ``num_clusters`` groups, as scikit-learn's ``AgglomerativeClustering(linkage='ward', connectivity=...)`` computes it and
    as ``rv_ward_groups`` does on the device (which keeps at most 2048 points; here every point is used).  Cluster r
    starts as point r with id r; while more than ``num_clusters`` live, the adjacent live pair smallest in (w, larger id,
    smaller id) merges into id n + step, w = |mean_a - mean_b|^2 c_a c_b / (c_a + c_b) in float64.  The groups are numbered
    by ascending smallest member; with fewer points than groups every point is its own group."""
    p = np.asarray(point_cloud, np.float32).astype(np.float64).reshape(-1, 3)
    n, c = len(p), int(num_clusters)
    if n <= c:
        return np.arange(n, dtype=np.int64)
    adj, _, _ = ward_graph(p, n_neighbors)
    mean, total, cnt, cid = p.copy(), p.copy(), np.ones(n), np.arange(n)
    live = np.ones(n, bool)
    owner = np.arange(n)                      # the slot of every point's cluster; a cluster lives in its smallest member's slot
    best_w, best = np.full(n, np.inf), np.full(n, -1, np.int64)

    def scan(t):
        nb = np.flatnonzero(adj[t])
        if not len(nb):
            return np.inf, -1
        w = _ward_dist(mean, cnt, t, nb)
        o = np.lexsort((np.minimum(cid[t], cid[nb]), np.maximum(cid[t], cid[nb]), w))[0]
        return w[o], nb[o]

    for t in range(n):
        best_w[t], best[t] = scan(t)
    for step in range(n - c):
        cand = np.flatnonzero(live & (best >= 0))
        if not len(cand):
            raise RuntimeError('ward_labels: no adjacent pair left (the graph is not connected)')
        ids, pid = cid[cand], cid[best[cand]]
        who = cand[np.lexsort((cand, np.minimum(ids, pid), np.maximum(ids, pid), best_w[cand]))[0]]
        keep, dead = sorted((int(who), int(best[who])))
        adj[keep] |= adj[dead]
        adj[keep, [keep, dead]] = False
        nb = np.flatnonzero(adj[keep])
        adj[nb, dead], adj[nb, keep], adj[dead] = False, True, False
        total[keep] = total[keep] + total[dead]
        cnt[keep] = cnt[keep] + cnt[dead]
        mean[keep] = total[keep] / cnt[keep]
        cid[keep], live[dead] = n + step, False
        owner[owner == dead] = keep
        best_w[keep], best[keep] = np.inf, -1
        if len(nb):
            w = _ward_dist(mean, cnt, keep, nb)
            o = np.lexsort((cid[nb], w))[0]
            best_w[keep], best[keep] = w[o], nb[o]
            gone = (best[nb] == keep) | (best[nb] == dead)
            better = ~gone & (w < best_w[nb])      # (equal w: the older pair has the smaller ids)
            best_w[nb[better]], best[nb[better]] = w[better], keep
            for t in nb[gone]:
                best_w[t], best[t] = scan(t)
    number = np.cumsum(live) - 1
    return number[owner].astype(np.int64)
