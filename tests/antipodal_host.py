"""NumPy restatement of rv_policy_antipodal (csrc/rv_dev_grasp_sampler.h), for the tests.

Float32 where the device works in float32, float64 where it works in float64, and a NumPy Philox4x32-10 for the
pair keys.  ``sample`` returns every intermediate the tests compare (edges, normals, w_max, the valid and the
passing pair sets, the chosen pair and the status), plus the pairs whose decisions are borderline: edge pixels
whose gradient magnitude lies within 1e-5 relative of the threshold.
"""
import math

import numpy as np

RV_STREAM_GRASP = 5
RV_STREAM_RANDOM = 2
DRAW_CTR = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (rv_dev_math.h), vectorised over uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = [np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & np.uint64(M32)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & np.uint64(M32)
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(M32)
    return c0, c1, c2, c3


def random_action_grasp(seed, gid, macro_index, low, high):
    """rv_policy_random for a Grasp4DofEnv (rv_dev_env.h random_action), float32."""
    o = philox(0, macro_index, gid, RV_STREAM_RANDOM, seed & M32, seed >> 32)
    u = [np.float32(int(x) >> 8) * np.float32(5.9604644775390625e-8) for x in o]
    a = [np.float32(-1.0) + np.float32(2.0) * x for x in u]
    out = [np.float32(low[k]) + (np.float32(high[k]) - np.float32(low[k])) * (np.float32(0.5) * (a[k] + np.float32(1.0))) for k in range(3)]
    out.append(np.float32(np.pi) * (a[3] + np.float32(1.0)))
    return np.array(out, np.float32)


def gaussian_weights(sigma):
    """(radius, w[0..radius]) of scipy.ndimage.gaussian_filter1d, float64 -> float32."""
    if sigma <= 1e-15:
        return 0, np.ones(1, np.float32)
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi /= phi.sum()
    return radius, phi[radius:].astype(np.float32)


def _reflect(i, n):
    p = 2 * n
    i = np.mod(i, p)
    return np.where(i < n, i, p - 1 - i)


def gaussian_filter(img, radius, w):
    """Separable, axis 0 then axis 1, 'reflect', float32 accumulation in the device's order."""
    img = np.asarray(img, np.float32)
    h, wd = img.shape
    out = img
    for axis, n in ((0, h), (1, wd)):
        idx = np.arange(n)
        take = (lambda a, j: a[j, :]) if axis == 0 else (lambda a, j: a[:, j])
        acc = out * w[0]
        for k in range(radius, 0, -1):
            acc = acc + (take(out, _reflect(idx - k, n)) + take(out, _reflect(idx + k, n))) * w[k]
        out = acc.astype(np.float32)
    return out


def pil_coeffs(in_size, out_size):
    """Pillow's BILINEAR resampling matrix [out, in] (Resample.c precompute_coeffs, triangle filter), float64."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = filterscale
    m = np.zeros((out_size, in_size))
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / filterscale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = np.array([max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)])
        ww = k.sum()
        if ww != 0.0:
            k = k / ww
        m[xx, xmin:xmin + xmax] = k
    return m


def pil_resize(img, rate):
    """PIL BILINEAR resize to int(W / rate) x int(H / rate) of a float32 image (horizontal, then vertical)."""
    img = np.asarray(img, np.float32)
    if rate == 1:
        return img.copy()
    h, w = img.shape
    hd, wd = int(h / rate), int(w / rate)
    tmp = (img.astype(np.float64) @ pil_coeffs(w, wd).T).astype(np.float32)
    return (pil_coeffs(h, hd) @ tmp.astype(np.float64)).astype(np.float32)


def np_grad(a):
    a = np.asarray(a, np.float32)
    return np.gradient(a)


def project_width(fx, cx, gripper_width, depth):
    """|Camera.project_point([W, 0, D]) - project_point([0, 0, D])| (camera.py:170-193, rounded pixels)."""
    if gripper_width <= 0:
        return np.inf
    u2 = np.round((gripper_width * fx + depth * cx) / depth)
    u1 = np.round((depth * cx) / depth)
    return float(abs(int(np.int16(u2)) - int(np.int16(u1))))


def bset_of(out):
    return set(map(tuple, out['borderline_pixels'].tolist()))


def sample(image, params, fx, cx, seed=0, gid=0, macro_index=0, max_edges=4096, borderline_rel=1e-5):
    """One env.  ``image`` [H, W] float32 depth; ``params`` a dict of the SAMPLER keys + GRIPPER_WIDTH.
    Returns a dict (see the module docstring)."""
    image = np.asarray(image, np.float32)
    H, W = image.shape
    p = params
    crop = p['CROP'] if p.get('CROP') is not None else [0, 0, H, W]
    r0, c0, r1, c1 = [int(v) for v in crop]
    rate = int(p['DOWNSAMPLE_RATE'])
    cone = np.float32(math.cos(math.atan(p['FRICTION_COEF'])))
    radius, w = gaussian_weights(p['DEPTH_GRAD_GAUSSIAN_SIGMA'])
    filt = gaussian_filter(image[r0:r1, c0:c1], radius, w)
    down = pil_resize(filt, rate)
    gx, gy = np_grad(down)
    mag = np.sqrt(gx.astype(np.float64) ** 2 + gy.astype(np.float64) ** 2)
    thr = float(np.float32(p['DEPTH_GRAD_THRESH']))
    is_edge = (mag > thr) | (down == 0)
    border = (np.abs(mag - thr) <= borderline_rel * thr) & (down != 0)
    ij = np.argwhere(is_edge)
    edges = rate * ij
    out = {'filtered': filt, 'down': down, 'edges': edges, 'borderline_pixels': rate * np.argwhere(border),
           'mag': mag, 'max_filtered': float(filt.max())}
    out['n_borderline'] = int(border.sum())
    E = len(edges)
    if E == 0:
        out.update(status=0, normals=np.zeros((0, 2), np.float32))
        return out
    if E > max_edges:
        out.update(status=-3)
        return out
    dy, dx = np_grad(filt)
    ndy, ndx = dy[edges[:, 0], edges[:, 1]], dx[edges[:, 0], edges[:, 1]]
    nn = np.sqrt(ndy * ndy + ndx * ndx).astype(np.float32)
    zero = nn == 0
    nn[zero] = 1
    normals = np.stack([ndy / nn, ndx / nn], 1).astype(np.float32)
    normals[zero] = [1.0, 0.0]
    out['normals'] = normals
    dmax = float(np.float32(filt.max())) + float(np.float32(p['MIN_DEPTH_OFFSET']))
    wmax = project_width(float(np.float32(fx)), float(np.float32(cx)), float(np.float32(p['GRIPPER_WIDTH'])), dmax)
    out['w_max'] = wmax
    ip = (normals[:, None, 0] * normals[None, :, 0] + normals[:, None, 1] * normals[None, :, 1]).astype(np.float32)
    d2 = ((edges[:, None, :] - edges[None, :, :]) ** 2).sum(-1)
    valid = (ip < -cone) & (d2 > 0) & (d2 < (wmax * wmax if np.isfinite(wmax) else np.inf))
    va, vb = np.nonzero(valid)
    # pairs whose validity is decided within 1e-6 of the cone (float32 here and on the device, float64 in the reference)
    near = np.abs(ip + cone) < 1e-6
    na_, nb_ = np.nonzero(near & (d2 > 0))
    out['borderline_pairs'] = set(zip(map(tuple, edges[na_].tolist()), map(tuple, edges[nb_].tolist())))
    out['valid'] = set(zip(map(tuple, edges[va].tolist()), map(tuple, edges[vb].tolist())))
    out['valid_idx'] = (va, vb)
    if len(va) == 0:
        out.update(status=-1, passing=set(), borderline_before_choice=bool(out['borderline_pairs']) or bool(bset_of(out)))
        return out
    # step 8 for every valid pair
    v = (edges[vb] - edges[va]).astype(np.float32)
    v = v / np.sqrt((v * v).sum(1)).astype(np.float32)[:, None]
    d1 = -(normals[va, 0] * v[:, 0] + normals[va, 1] * v[:, 1])
    d2_ = normals[vb, 0] * v[:, 0] + normals[vb, 1] * v[:, 1]
    fc = (d1 > cone) & (d1 <= 1) & (d2_ > cone) & (d2_ <= 1)
    # ... and force-closure decisions within 1e-6 of the cone or of 1 (where the reference's arccos turns NaN)
    fb = np.minimum.reduce([np.abs(d1 - cone), np.abs(d2_ - cone), np.abs(d1 - 1), np.abs(d2_ - 1)]) < 1e-6
    out['borderline_pairs'] |= set(zip(map(tuple, edges[va[fb]].tolist()), map(tuple, edges[vb[fb]].tolist())))
    gxc = 0.5 * (edges[va, 1] + edges[vb, 1] + 2 * c0)
    gyc = 0.5 * (edges[va, 0] + edges[vb, 0] + 2 * r0)
    dist = np.minimum.reduce([np.abs(r0 - gyc), np.abs(c0 - gxc), np.abs(gyc - r1), np.abs(gxc - c1)])
    ok = fc & (dist >= np.float32(p['MIN_DIST_FROM_BOUNDARY']))
    wh, ww = float(np.float32(p['DEPTH_SAMPLE_WINDOW_HEIGHT'])), float(np.float32(p['DEPTH_SAMPLE_WINDOW_WIDTH']))
    cdepth = np.zeros(len(va), np.float32)
    for k in np.nonzero(ok)[0]:
        win = image[int(gyc[k] - wh):int(gyc[k] + wh), int(gxc[k] - ww):int(gxc[k] + ww)]
        cd = np.min(win)
        if cd == 0 or np.isnan(cd):
            ok[k] = False
        cdepth[k] = cd
    out['passing'] = set(zip(map(tuple, edges[va[ok]].tolist()), map(tuple, edges[vb[ok]].tolist())))
    # order: Philox keys of (pixel i, pixel j)
    pix_a = (r0 + edges[va, 0]) * W + c0 + edges[va, 1]
    pix_b = (r0 + edges[vb, 0]) * W + c0 + edges[vb, 1]
    word3 = (RV_STREAM_GRASP << 24) | (macro_index & 0xFFFFFF)
    keys = philox(pix_a, pix_b, np.full(len(va), gid), np.full(len(va), word3), seed & M32, seed >> 32)[0].astype(np.uint64)
    comp = (keys << np.uint64(32)) | (va * E + vb).astype(np.uint64)
    order = np.argsort(comp, kind='stable')
    ranks_ok = np.nonzero(ok[order])[0]
    K = min(int(p['MAX_REJECTION_SAMPLES']), len(va))
    # borderline: a pair touching a borderline pixel that ranks at or before the choice
    bset = set(map(tuple, out['borderline_pixels'].tolist()))
    first = int(ranks_ok[0]) if len(ranks_ok) else len(order)
    bpairs = out['borderline_pairs']
    out['borderline_before_choice'] = bool(bpairs) and any(
        tuple(edges[va[order[k]]]) in bset or tuple(edges[vb[order[k]]]) in bset or
        (tuple(edges[va[order[k]]]), tuple(edges[vb[order[k]]])) in bpairs for k in range(min(first + 1, len(order)))) or any(
        tuple(edges[va[order[k]]]) in bset or tuple(edges[vb[order[k]]]) in bset for k in range(min(first + 1, len(order))))
    if len(ranks_ok) == 0 or ranks_ok[0] >= K:
        out.update(status=-2)
        return out
    k = order[ranks_ok[0]]
    a, b = int(va[k]), int(vb[k])
    cd = cdepth[k]
    u = np.float32(int(philox(DRAW_CTR, DRAW_CTR, gid, word3, seed & M32, seed >> 32)[0]) >> 8) * np.float32(5.9604644775390625e-8)
    lo = cd + np.float32(p['MIN_DEPTH_OFFSET'])
    hi = cd + np.float32(p['MAX_DEPTH_OFFSET'])
    g = np.array([edges[a, 1] + c0, edges[a, 0] + r0, edges[b, 1] + c0, edges[b, 0] + r0, lo + u * (hi - lo)], np.float32)
    out.update(status=1, pair=(tuple(edges[a].tolist()), tuple(edges[b].tolist())), grasp=g, center_depth=float(cd))
    return out


def synth_image(spec):
    """A small synthetic depth image from its parameters (the golden records only these): a tilted plane at
    spec['plane'] = [depth, d/drow, d/dcol], boxes [r0, c0, r1, c1, depth] and cylinders [row, col, radius, depth]
    (a rounded top: depth + 0.3 radius_m (1 - sqrt(1 - s^2))), 'zero_background' (no plane outside the objects) and
    'noise' (Gaussian sigma, numpy seed)."""
    h, w = spec['shape']
    rr, cc = np.mgrid[0:h, 0:w].astype(np.float64)
    d0, dr, dc = spec['plane']
    img = d0 + dr * rr + dc * cc
    if spec.get('zero_background'):
        img[:] = 0.0
    for r0, c0, r1, c1, z in spec.get('boxes', []):
        img[r0:r1, c0:c1] = z
    for r, c, rad, z in spec.get('cylinders', []):
        s2 = ((rr - r) ** 2 + (cc - c) ** 2) / float(rad * rad)
        inside = s2 < 1.0
        img[inside] = (z + 0.03 * (1.0 - np.sqrt(1.0 - np.minimum(s2, 1.0))))[inside]
    if spec.get('noise'):
        sigma, seed = spec['noise']
        img = img + np.random.RandomState(seed).normal(0.0, sigma, img.shape) * (img > 0)
    return img.astype(np.float32)
