"""NumPy restatement of csrc/rv_dev_grasp_refine.h (rv_grasp_refine), for the tests: float32, operation for
operation, every product and sum rounded on its own.

Built on what exists: the normals (``normal_pair``: logr, sincosr with its two emulated fused multiply-adds), ``fclampr``
and the ranking (``cem_key`` / ``cem_rank``) of tests/cem_host.py, the Philox block of tests/antipodal_host.py, and the
boundary and depth-window checks in the form ``antipodal_host.sample`` writes them (there they are inlined over the valid
pairs; ``check_center`` is the same arithmetic for one centre that need not be a half-integer).

``as_4dof`` restates ap_grasp_4dof (rv_dev_grasp_sampler.h).  Its position is float32 sums, products and quotients and is
restated exactly; its yaw goes through the device's libm (atan2f, cosf, sinf), whose last bits no host restatement owns,
so the yaw is evaluated here in float64 from the float32 row and compared within YAW_TOL (below), as the tests of
rv_policy_antipodal_multi compare that conversion with Grasp2D.as_4dof (there within 1e-4).

Bounds used by tests/test_grasp_refine_host.py for the child geometry against a float64 evaluation of the same formulas.
u = 2^-24 is the relative rounding error of one float32 operation; M = 1024 bounds every coordinate-sized intermediate
(coordinates up to 512 px plus a displacement of the same size), so one rounding of such a value is at most u M = 6.1e-5.

* Centre.  The parent's centre gx = 0.5 (x1 + x2) rounds once (the halving is exact); cx = gx + sigma z0 rounds the
  product (u |sigma z0| <= u M) and the sum; the child's ends cx -+ bx round once each, with errors e1, e2, and the
  centre recovered from the row in float64 is cx + (e1 + e2) / 2.  Four roundings of coordinate size:
      CENTER_TOL = 4 u M = 2.44e-4 px   per axis.
* Half axis.  a = 0.5 (p2 - p1) rounds once per component (u L each, L = |a| <= 512).  (s, c) of sincosr are within
  2^-23 of the true sine and cosine (rv_dev_math.h CONTRACT), so the rotated vector is within 2 * 2^-23 L of the true
  rotation of a, in length and across it; each component of b = (c ax - s ay, s ax + c ay) adds three roundings of at most
  u L; the half axis recovered from the row is b + (e2 - e1) / 2 with |e| <= u M.  Adding the components' errors as
  sqrt(2) times the per-component error:
      LEN_TOL(L)   = 2^-22 L + sqrt(2) (4 u L + u M)            <= 3.3e-4 px at L = 512
      ANGLE_TOL(L) = LEN_TOL(L) / L                              radians: the same error seen across the axis
  (a short axis turns the end-point rounding u M into a larger angle: 2.9e-5 rad at L = 3 px).
* YAW_TOL = 1e-5 rad (modulo 2 pi).  angle = atan2f(dy, dx): <= 2 ulp of pi = 4.8e-7; phi = angle + pi/2 rounds once more
  (2.4e-7); cosf / sinf of it: <= 2 ulp (2.4e-7) plus the argument's 7.2e-7; m00 and m10 are two products and a sum of
  those with rotation entries (<= 1 in magnitude): <= 2.2e-6 each; the final atan2f of a vector of length r turns that into
  <= 3.1e-6 / r + 4.8e-7.  For the top-down cameras of the project r >= 0.9: 3.9e-6, rounded up to 1e-5."""
import numpy as np

import cem_host
from antipodal_host import philox, M32

F = np.float32
RV_STREAM_GRASP_REFINE = 11
MAX_ITERATION, MAX_MACRO_INDEX, MAX_SAMPLES = 1 << 26, 1 << 24, 64
RV_AP_OK = 1
FLT_MAX = F(3.402823466e38)
U = 2.0 ** -24
M_COORD = 1024.0
CENTER_TOL = 4 * U * M_COORD
YAW_TOL = 1e-5


def len_tol(L):
    return 2.0 ** -22 * L + np.sqrt(2.0) * (4 * U * L + U * M_COORD)


def angle_tol(L):
    return len_tol(L) / L


def counter_words(macro_index, iteration, seed, gid, j):
    """(c0, c1, c2, c3) of output row j (arrays broadcast)"""
    assert 0 <= iteration < MAX_ITERATION and 0 <= macro_index < MAX_MACRO_INDEX and np.max(j) < MAX_SAMPLES
    j = np.asarray(j, np.uint64)
    c0 = (np.uint64(iteration) << np.uint64(6)) | j
    return c0, np.full_like(c0, seed & M32), np.full_like(c0, gid), np.full_like(c0, (RV_STREAM_GRASP_REFINE << 24) | macro_index)


def normals(world_seed, gid, macro_index, iteration, seed, j):
    """the four normals of output rows j -> float32 [..., 4]"""
    c0, c1, c2, c3 = counter_words(macro_index, iteration, seed, gid, j)
    o = philox(c0, c1, c2, c3, world_seed & M32, world_seed >> 32)
    z0, z1 = cem_host.normal_pair(o[0], o[1])
    z2, z3 = cem_host.normal_pair(o[2], o[3])
    return np.stack([z0, z1, z2, z3], axis=-1).astype(F)


def crop_of(sampler, H, W):
    crop = sampler['CROP'] if sampler.get('CROP') is not None else [0, 0, H, W]
    return [int(v) for v in crop]


def check_center(image, sampler, ux, uy):
    """ap_check_center: (passes, centre depth) for the centre (ux, uy), float32 scalars"""
    H, W = image.shape
    r0, c0, r1, c1 = crop_of(sampler, H, W)
    ux, uy = F(ux), F(uy)
    dist = np.abs(F(r0) - uy)
    for other in (np.abs(F(c0) - ux), np.abs(uy - F(r1)), np.abs(ux - F(c1))):
        dist = min(dist, other)
    if dist < F(sampler['MIN_DIST_FROM_BOUNDARY']):
        return False, F(0)
    wh, ww = float(F(sampler['DEPTH_SAMPLE_WINDOW_HEIGHT'])), float(F(sampler['DEPTH_SAMPLE_WINDOW_WIDTH']))
    y0, y1 = int(float(uy) - wh), int(float(uy) + wh)
    x0, x1 = int(float(ux) - ww), int(float(ux) + ww)
    y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H), min(x1, W)
    if y1 <= y0 or x1 <= x0:
        return False, F(0)
    win = image[y0:y1, x0:x1]
    if np.isnan(win).any():
        return False, F(0)
    cd = F(win.min())
    if cd == 0:
        return False, F(0)
    return True, cd


def sincos_arg(x):
    return cem_host.fclampr(np.asarray(x, F), -1.0e4, 1.0e4)


def child(image, sampler, g, z, sigmas):
    """gr_child: parent row g [5], normals z [4], sigmas (centre, angle, depth) -> (accepted, row float32 [5])"""
    g, z = np.asarray(g, F), np.asarray(z, F)
    sc, sa, sd = [F(v) for v in sigmas]
    H, W = image.shape
    r0, c0, r1, c1 = crop_of(sampler, H, W)
    with np.errstate(all='ignore'):
        gx, gy = F(0.5) * (g[0] + g[2]), F(0.5) * (g[1] + g[3])
        ax, ay = F(0.5) * (g[2] - g[0]), F(0.5) * (g[3] - g[1])
        cx, cy = gx + sc * z[0], gy + sc * z[1]
        s, c = cem_host.sincosr(sincos_arg(sa * z[2]).reshape(1))
        s, c = s[0], c[0]
        bx, by = c * ax - s * ay, s * ax + c * ay
        out = np.zeros(5, F)
        out[0], out[1], out[2], out[3] = cx - bx, cy - by, cx + bx, cy + by
        ux, uy = F(0.5) * (out[0] + out[2]), F(0.5) * (out[1] + out[3])
        inside = ux >= F(c0) and ux <= F(c1) and uy >= F(r0) and uy <= F(r1)
        if not inside:
            return False, out
        ok, cd = check_center(image, sampler, ux, uy)
        if not ok:
            return False, out
        lo, hi = cd + F(sampler['MIN_DEPTH_OFFSET']), cd + F(sampler['MAX_DEPTH_OFFSET'])
        out[4] = cem_host.fclampr(np.asarray(g[4] + sd * z[3], F).reshape(1), lo, hi)[0]
        return bool(np.all(np.abs(out) <= FLT_MAX)), out


def rank(scores, cand):
    """input indices of the candidates (``cand`` bool [K]) in the order of rv_cem_refit, best first"""
    idx = np.nonzero(cand)[0]
    key = cem_host.cem_key(np.ascontiguousarray(scores, F)[idx]).astype(np.uint64)
    word = (key << np.uint64(32)) | idx.astype(np.uint64)
    return (np.sort(word) & np.uint64(M32)).astype(np.int32)


def as_4dof(cam_row, g):
    """ap_grasp_4dof of row g with the calibration ``cam_row`` = [fx, fy, cx, cy, skew, R (9, row major), t (3)] (one row
    of World.camera()): float32 [x, y, z] restated exactly, and the yaw in float64 (module docstring)"""
    k = np.asarray(cam_row, F)
    fx, fy, cx, cy, sk = k[0], k[1], k[2], k[3], k[4]
    R, t = k[5:14], k[14:17]
    g = np.asarray(g, F)
    with np.errstate(all='ignore'):
        u, v, z = F(0.5) * (g[0] + g[2]), F(0.5) * (g[1] + g[3]), g[4]
        yc = (v - cy) / fy
        xc = (u - cx - sk * yc) / fx
        q = [z * xc - t[0], z * yc - t[1], z - t[2]]
        xyz = [R[i] * q[0] + R[3 + i] * q[1] + R[6 + i] * q[2] for i in range(3)]
        angle = np.arctan2(float(g[3] - g[1]), float(g[2] - g[0]))
        phi = angle + 0.5 * np.pi
        m00 = float(R[0]) * np.cos(phi) + float(R[3]) * np.sin(phi)
        m10 = float(R[1]) * np.cos(phi) + float(R[4]) * np.sin(phi)
        yaw = np.arctan2(m10, m00) if np.hypot(m00, m10) > 8.881784197001252e-16 else 0.0
    return np.array(xyz, F), float(yaw)


def refine(depth, grasps, scores, n_elites, sigmas, sampler, count=None, status=None, world_seed=0, env_id_offset=0,
           macro_index=0, iteration=0, seed=0):
    """k_grasp_refine: depth [N, H, W], grasps [N, K, 5], scores [N, K], count / status [N] or None ->
    (grasps_out float32 [N, K, 5], parent int32 [N, K], count_out int32 [N])"""
    depth = np.ascontiguousarray(depth, F)
    grasps = np.ascontiguousarray(grasps, F)
    scores = np.ascontiguousarray(scores, F)
    N, K, _ = grasps.shape
    E = int(n_elites)
    assert 1 <= K <= MAX_SAMPLES and 1 <= E <= K
    out = grasps.copy()
    parent = np.tile(np.arange(K, dtype=np.int32), (N, 1))
    count_out = np.zeros(N, np.int32)
    j = np.arange(K)
    for n in range(N):
        cand = np.ones(K, bool)
        if status is not None:
            cand &= int(status[n]) == RV_AP_OK
        if count is not None:
            cand &= j < int(count[n])
        V = int(cand.sum())
        if V == 0:
            continue
        count_out[n] = K
        order = rank(scores[n], cand)
        Ep = min(E, V)
        z = normals(world_seed, env_id_offset + n, macro_index, iteration, seed, j)
        for row in range(K):
            if row < Ep:
                e = int(order[row])
                out[n, row], parent[n, row] = grasps[n, e], e
                continue
            e = int(order[(row - Ep) % Ep])
            ok, ch = child(depth[n], sampler, grasps[n, e], z[row], sigmas)
            if ok:
                out[n, row], parent[n, row] = ch, e
            else:
                out[n, row], parent[n, row] = grasps[n, e], -1 - e
    return out, parent, count_out
