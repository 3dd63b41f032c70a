"""NumPy restatement of rv_policy_antipodal_multi (csrc/rv_dev_grasp_sampler.h), for the tests: the reference's walk
``sample(depth, camera, num_samples)`` (image_grasp_sampler.py:303-375) over the key order of ``antipodal_host.sample``.

Built on that function's intermediates (edges, the valid pairs, the set passing the per-candidate checks); the pair
keys, the walk, the distance to the grasps accepted so far and the depth draws are restated here.  The distance makes
the NumPy calls the reference makes on arrays of the reference's dtypes -- the candidate a float64 row, the accepted
grasps rows of a float32 array, ``np.linalg.norm`` over the whole 2-D array of axes -- so that its quirks (the common
divisor, the float32 quotient, the NaN that accepts) are NumPy's own.
"""
import numpy as np

import antipodal_host as host

MAX_SAMPLES = 64


def grasp_dist(candidate, accepted):
    """Distance of a candidate [1, 5] float64 to the accepted grasps [n, 5] float32, weight of the angle term 1.0
    (the default the reference's ``_sample`` never overrides: ANGLE_DIST_WEIGHT is not used)."""
    c_axis = candidate[:, 2:4] - candidate[:, 0:2]
    c_axis = c_axis / np.linalg.norm(c_axis)
    c_center = 0.5 * (candidate[:, 0:2] + candidate[:, 2:4])
    a_axis = accepted[:, 2:4] - accepted[:, 0:2]
    a_axis = a_axis / np.linalg.norm(a_axis)          # one divisor for all rows, float32
    a_center = 0.5 * (accepted[:, 0:2] + accepted[:, 2:4])
    with np.errstate(invalid='ignore'):
        return np.linalg.norm(c_center - a_center, axis=-1) + 1.0 * np.arccos(np.sum(c_axis * a_axis, axis=-1))


def pair_keys(image_shape, params, edges, va, vb, seed, gid, macro_index):
    """composite keys (Philox key << 32 | a * E + b) of the ordered edge pairs (va, vb)"""
    H, W = image_shape
    crop = params['CROP'] if params.get('CROP') is not None else [0, 0, H, W]
    r0, c0 = int(crop[0]), int(crop[1])
    E = len(edges)
    pix_a = (r0 + edges[va, 0]) * W + c0 + edges[va, 1]
    pix_b = (r0 + edges[vb, 0]) * W + c0 + edges[vb, 1]
    word3 = (host.RV_STREAM_GRASP << 24) | (macro_index & 0xFFFFFF)
    keys = host.philox(pix_a, pix_b, np.full(len(va), gid), np.full(len(va), word3), seed & host.M32, seed >> 32)[0].astype(np.uint64)
    return (keys << np.uint64(32)) | (np.asarray(va) * E + np.asarray(vb)).astype(np.uint64)


def depth_draw(seed, gid, macro_index, k):
    """the uniform of accepted grasp k: Philox counter words (DRAW_CTR, DRAW_CTR - k), 24 bits, float32"""
    word3 = (host.RV_STREAM_GRASP << 24) | (macro_index & 0xFFFFFF)
    o = host.philox(host.DRAW_CTR, host.DRAW_CTR - k, gid, word3, seed & host.M32, seed >> 32)[0]
    return np.float32(int(o) >> 8) * np.float32(5.9604644775390625e-8)


def sample_multi(image, params, fx, cx, num_samples, seed=0, gid=0, macro_index=0, max_edges=4096, base=None):
    """One env, up to ``num_samples`` grasps.  Returns a dict: ``status`` (1 / 0 / -1 / -2 / -3), ``count``, ``grasps``
    float32 [K, 5] (None without a grasp), ``pairs`` (the accepted (p1, p2) in crop coordinates), ``walked`` (pairs
    consumed), ``draws`` (K_draws), ``order`` (indices into the valid list in walk order, cut after K_draws),
    ``borderline`` (a borderline pixel or pair at or before the last walked rank: the float32 / float64 decisions
    ``antipodal_host`` flags) and ``base``, the dict of ``antipodal_host.sample`` (computed here unless passed in: it does
    not depend on ``num_samples``)."""
    K = int(num_samples)
    assert 1 <= K <= MAX_SAMPLES
    image = np.asarray(image, np.float32)
    H, W = image.shape
    p = params
    if base is None:
        base = host.sample(image, p, fx, cx, seed=seed, gid=gid, macro_index=macro_index, max_edges=max_edges)
    out = {'base': base, 'count': 0, 'grasps': None, 'pairs': [], 'walked': 0, 'draws': 0, 'order': np.zeros(0, np.int64),
           'borderline': False}
    if base['status'] in (0, -3):
        out['status'] = base['status']
        out['borderline'] = bool(base.get('n_borderline', 0))
        return out
    edges = base['edges']
    va, vb = base['valid_idx']
    bpix = host.bset_of(base)
    bpairs = base['borderline_pairs']
    if len(va) == 0:
        out['status'] = -1
        out['borderline'] = bool(bpairs) or bool(bpix)
        return out
    crop = p['CROP'] if p.get('CROP') is not None else [0, 0, H, W]
    r0, c0 = int(crop[0]), int(crop[1])
    comp = pair_keys(image.shape, p, edges, va, vb, seed, gid, macro_index)
    order = np.argsort(comp, kind='stable')
    draws = min(int(p['MAX_REJECTION_SAMPLES']), len(va))
    out['draws'] = draws
    out['order'] = order[:draws]
    passing = base['passing']
    mgd = float(np.float32(p['MIN_GRASP_DIST']))
    wh, ww = float(np.float32(p['DEPTH_SAMPLE_WINDOW_HEIGHT'])), float(np.float32(p['DEPTH_SAMPLE_WINDOW_WIDTH']))
    grasps = np.zeros([K, 5], np.float32)
    n = 0
    walked = 0
    for rank in range(draws):
        if n >= K:
            break
        walked = rank + 1
        k = order[rank]
        pa, pb = tuple(edges[va[k]].tolist()), tuple(edges[vb[k]].tolist())
        if (pa, pb) not in passing:
            continue
        point1 = np.array([pa[1] + c0, pa[0] + r0])
        point2 = np.array([pb[1] + c0, pb[0] + r0])
        if n > 0:
            cand = np.expand_dims(np.r_[point1, point2, 0.0], 0)
            if np.min(grasp_dist(cand, grasps[:n, :])) <= mgd:
                continue
        gc = 0.5 * (point1 + point2)
        cd = np.min(image[int(gc[1] - wh):int(gc[1] + wh), int(gc[0] - ww):int(gc[0] + ww)])
        lo = cd + np.float32(p['MIN_DEPTH_OFFSET'])
        hi = cd + np.float32(p['MAX_DEPTH_OFFSET'])
        row = np.array([point1[0], point1[1], point2[0], point2[1], lo + depth_draw(seed, gid, macro_index, n) * (hi - lo)], np.float32)
        if n == 0:
            grasps[:, :] = row
        else:
            grasps[n] = row
        out['pairs'].append((pa, pb))
        n += 1
    out['walked'] = walked
    # borderline decisions among what the walk saw: a walked pair on a borderline pixel, or a borderline pair (valid
    # here or not) whose key does not come after the last walked one
    last = comp[order[walked - 1]] if walked else np.uint64(0)
    flag = False
    for rank in range(walked):
        k = order[rank]
        if tuple(edges[va[k]].tolist()) in bpix or tuple(edges[vb[k]].tolist()) in bpix:
            flag = True
            break
    if not flag and bpairs:
        index = {tuple(e): j for j, e in enumerate(edges.tolist())}
        ba = np.array([index[a] for a, b in bpairs])
        bb = np.array([index[b] for a, b in bpairs])
        flag = bool((pair_keys(image.shape, p, edges, ba, bb, seed, gid, macro_index) <= last).any())
    out['borderline'] = flag
    out['count'] = n
    out['status'] = 1 if n else -2
    out['grasps'] = grasps if n else None
    return out
