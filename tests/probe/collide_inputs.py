"""Shared inputs of the collision / wave probe: tests/test_collide_probe.py holds the host compile of rv_dev_collide.h
to float64 references on them, tests/test_gpu_collide_probe.py holds the gfx950 build to the host compile on the same
arrays.  Fixed seeds; every value is a float32 (the float64 references see exactly what the code under test sees)."""
import functools

import numpy as np
from scipy.spatial import ConvexHull

F = np.float32
MAXV = 16
# half extents of the shipped boxes (robovat_amd/scenes.py: bodies, wall, table slab, arm collider boxes)
BOX_HALVES = ((0.035, 0.03, 0.03), (0.014, 0.014, 0.014), (0.012, 0.035, 0.015), (0.03, 0.05, 0.03), (0.008, 0.006, 0.035),
              (0.02, 0.65, 0.4), (0.38, 0.61, 0.02))


def pack_hulls(hulls):
    """[n] arrays [k, 3] -> (verts [n, 48] float32, counts [n] int32); the rows past a hull's count are NaN: whoever
    reads one spoils its result."""
    verts = np.full((len(hulls), MAXV, 3), np.nan, F)
    cnt = np.zeros(len(hulls), np.int32)
    for i, h in enumerate(hulls):
        h = np.asarray(h, F).reshape(-1, 3)
        assert 1 <= len(h) <= MAXV
        verts[i, :len(h)] = h
        cnt[i] = len(h)
    return verts.reshape(len(hulls), 3 * MAXV), cnt


def rot(rng):
    q = rng.randn(4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def unit(rng):
    u = rng.randn(3)
    return u / np.linalg.norm(u)


def box(h):
    return np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)


def cylinder16(r, hh):
    th = np.arange(8) * 2 * np.pi / 8
    ring = np.stack([r * np.cos(th), r * np.sin(th)], 1)
    return np.concatenate([np.concatenate([ring, np.full((8, 1), hh)], 1), np.concatenate([ring, np.full((8, 1), -hh)], 1)])


def sphere16(r, rng):
    u = rng.randn(16, 3)
    return r * u / np.linalg.norm(u, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------- support_v --
@functools.lru_cache(maxsize=None)
def support_cases():
    """(verts [n, 48], cnt [n], dirs [n, 3], tags [n]).  Shuffled once, so that the four rows of a wave hold different
    hulls with different counts."""
    rng = np.random.RandomState(101)
    hulls, dirs, tags = [], [], []

    def put(h, d, tag):
        hulls.append(np.asarray(h, F)); dirs.append(np.asarray(d, F)); tags.append(tag)
    for n in (1, 2, 3, 8, 15, 16):
        for _ in range(12):
            put(rng.randn(n, 3) * 0.03, unit(rng), 'random')
        for _ in range(6):                       # the maximum at index 0, and at index n - 1 (for n < 16 the clamped
            d = unit(rng)                        # lanes n..15 then all hold the winner)
            for where in (0, n - 1):
                h = rng.randn(n, 3) * 0.01
                h[where] += 0.1 * d
                put(h, d, 'max_first' if where == 0 else 'max_last')
        for _ in range(6):                       # exact ties between distinct indices: duplicated vertices on top
            if n < 2:
                continue
            d = unit(rng)
            h = rng.randn(n, 3) * 0.01
            j, k = sorted(rng.choice(n, 2, replace=False))
            h[j] += 0.1 * d
            h[k] = h[j]
            if n >= 8:
                h[n - 1] = h[j]
            put(h, d, 'tie')
        put(np.tile(rng.randn(1, 3) * 0.03, (n, 1)), unit(rng), 'all_equal')
        put(rng.randn(n, 3) * 0.03, np.zeros(3), 'dir_zero')
        # projections of +0 and -0 tying: (-1,-1,-1) . (+0,+0,+0) = -0, (1,1,1) . (+0,+0,+0) = +0, and both orders
        sg = np.where(np.arange(n) % 2 == 0, -1.0, 1.0)[:, None]
        put(sg * np.ones((n, 3)), np.zeros(3), 'signed_zero')
        put(-sg * np.ones((n, 3)), np.zeros(3), 'signed_zero')
        put(sg * np.ones((n, 3)), -np.zeros(3), 'signed_zero')
    order = np.random.RandomState(102).permutation(len(hulls))
    verts, cnt = pack_hulls([hulls[i] for i in order])
    return verts, cnt, np.stack([dirs[i] for i in order]).astype(F), [tags[i] for i in order]


# ---------------------------------------------------------------------------------------------- sub-simplex solvers --
@functools.lru_cache(maxsize=None)
def simplex_cases(nv):
    """[n, nv, 3] float32 simplices (nv = 2, 3, 4) at 1 cm to 10 cm scale, the origin placed over every feature: a point
    of the feature's relative interior plus a step into the feature's normal cone.  Then the degenerate ones."""
    rng = np.random.RandomState(200 + nv)
    out = []
    subsets = [s for s in range(1, 1 << nv)]
    for rep in range(40):
        for sub in subsets + ([0] if nv == 4 else []):         # 0: the origin inside the tetrahedron
            scale = 10.0 ** rng.uniform(-2, -1)
            W = rng.randn(nv, 3) * scale
            idx = [k for k in range(nv) if sub >> k & 1]
            if sub == 0:
                lam = rng.dirichlet(np.ones(nv) * 2.0)
                out.append(W - lam @ W)
                continue
            lam = rng.dirichlet(np.ones(len(idx)) * 2.0)
            p = lam @ W[idx]
            # a direction in the normal cone of the feature: away from the rest of the simplex, orthogonal to the feature
            rest = [k for k in range(nv) if k not in idx]
            d = p - W[rest].mean(0) if rest else rng.randn(3)
            for k in idx[1:]:
                e = W[k] - W[idx[0]]
                d = d - e * (d @ e) / (e @ e) if len(idx) == 2 else d
            if len(idx) == 3:
                nrm = np.cross(W[idx[1]] - W[idx[0]], W[idx[2]] - W[idx[0]])
                d = nrm * np.sign(d @ nrm)
            d = d / np.linalg.norm(d)
            out.append(W - (p + d * scale * rng.uniform(0.05, 1.0)))
    for rep in range(24):                                      # random placement as well
        scale = 10.0 ** rng.uniform(-2, -1)
        out.append(rng.randn(nv, 3) * scale + rng.randn(3) * scale)
    for rep in range(12):                                      # degenerate
        scale = 10.0 ** rng.uniform(-2, -1)
        o = rng.randn(3) * scale
        if nv == 2:
            p = rng.randn(3) * scale
            out.append(np.stack([p, p]) + o)                   # zero-length segment
        elif nv == 3:
            p, e = rng.randn(3) * scale, rng.randn(3) * scale
            t = rng.uniform(-1, 2, 3)
            out.append(p + t[:, None] * e + o * 0.3)           # collinear triangle (up to float32 rounding)
        else:
            p, e1, e2 = rng.randn(3) * scale, rng.randn(3) * scale, rng.randn(3) * scale
            t = rng.uniform(-1, 1, (4, 2))
            out.append(p + t[:, :1] * e1 + t[:, 1:] * e2 + o * 0.3)     # flat tetrahedron
    return np.asarray(out, F)


# ------------------------------------------------------------------------------------------------------------ gjk_epa --
# ('moved:<class>': the separated pairs of <class> with B moved a little, for the simplex cache)
GJK_CLASSES = ('random', 'boxes', 'cylinders', 'point', 'segment', 'quad', 'far', 'tiny', 'parallel', 'duplicates')
PAIRS_PER_CLASS = 256


def _hull(cls, rng, second=False):
    if cls in ('random', 'far'):
        return rng.randn(rng.randint(4, 17), 3) * [0.03, 0.02, 0.025]
    if cls == 'tiny':
        return rng.randn(rng.randint(4, 17), 3) * 1e-3
    if cls == 'boxes':
        k = rng.randint(0, len(BOX_HALVES) - (2 if second else 0))
        return box(BOX_HALVES[k]) @ rot(rng).T
    if cls == 'cylinders':
        return cylinder16(rng.uniform(0.01, 0.03), rng.uniform(0.005, 0.03)) @ rot(rng).T
    if cls == 'duplicates':
        h = rng.randn(rng.randint(4, 9), 3) * 0.03
        return np.concatenate([h, h[rng.randint(0, len(h), rng.randint(1, 9))]])
    if cls == 'point':
        return rng.randn(1, 3) * 0.01
    if cls == 'segment':
        return rng.randn(2, 3) * 0.03
    if cls == 'quad':
        return (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0.0]]) * rng.uniform(0.01, 0.04, 3)) @ rot(rng).T
    raise KeyError(cls)


@functools.lru_cache(maxsize=None)
def gjk_pairs(cls, overlapping):
    """PAIRS_PER_CLASS pairs of class `cls`: a list of (A [nA, 3], B [nB, 3], guess [3]) in float32.  B is pushed along a
    random direction u until the two support planes across u are a gap apart (separated), or until the origin lies a
    chosen step inside the difference body (overlapping); what the pair then IS -- its distance or depth -- is for the
    float64 certificate of the test to say, not for this generator."""
    if cls.startswith('moved:'):
        return _moved(gjk_pairs(cls[6:], overlapping), 77)
    rng = np.random.RandomState(1000 + 2 * GJK_CLASSES.index(cls) + int(overlapping))
    out = []
    for i in range(PAIRS_PER_CLASS):
        if cls == 'parallel':
            A = B = None
        elif cls in ('point', 'segment', 'quad'):
            A = _hull(cls, rng)
            # against a solid hull, and (separated only: the overlap of two flat sets has no depth) against another flat one
            B = _hull(('point', 'segment', 'quad')[rng.randint(3)], rng) if (not overlapping and i % 2) else _hull('random', rng)
        else:
            A, B = _hull(cls, rng), _hull(cls, rng, second=True)
        small = 1e-3 if cls == 'tiny' else 1.0
        if cls == 'parallel':
            R = rot(rng)
            ha, hb = rng.uniform(0.01, 0.04, 3), rng.uniform(0.01, 0.04, 3)
            s = rng.uniform(0, 0.004) * (-1 if overlapping else 1)
            off = np.array([rng.uniform(-1, 1) * ha[0], rng.uniform(-1, 1) * ha[1], -(ha[2] + hb[2] + s)])
            A, B = box(ha) @ R.T, (box(hb) + off) @ R.T
            c = rng.randn(3) * 0.05
            A, B = A + c, B + c
        else:
            u = unit(rng)
            B = B - B.mean(0) + A.mean(0)
            if overlapping:
                # the difference body A - B now holds the origin (both hulls hold the common centroid); the ray from it
                # along u leaves the body at rho: moving B by (rho - p) u leaves the origin p short of that exit
                eq = ConvexHull((A[:, None, :] - B[None, :, :]).reshape(-1, 3)).equations
                along = eq[:, :3] @ u
                rho = (-eq[:, 3][along > 1e-9] / along[along > 1e-9]).min()
                B = B + u * (rho - min(rng.uniform(0.0001, 0.02) * small, 0.9 * rho))
            else:
                s = 10.0 ** rng.uniform(-4, -1.5) * small
                # (min over A of u.a) - (max over B of u.b) = s
                B = B + u * ((A @ u).min() - (B @ u).max() - s)
            if cls == 'far':
                c = unit(rng) * 1.5
                A, B = A + c, B + c
        A, B = A.astype(F), B.astype(F)
        true_dir = A.astype(np.float64).mean(0) - B.astype(np.float64).mean(0)
        guess = (true_dir, np.zeros(3), -true_dir, rng.randn(3))[i % 4]
        out.append((A, B, np.asarray(guess, F)))
    return out


def _moved(pairs, seed):
    """The pairs with B after a small rigid motion about its centroid: at most 2 mm and 2 degrees (the simplex cache's case)"""
    rng = np.random.RandomState(seed)
    out = []
    for A, B, g in pairs:
        ax = unit(rng); ang = np.deg2rad(rng.uniform(-2, 2))
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        c = B.astype(np.float64).mean(0)
        B2 = (B.astype(np.float64) - c) @ R.T + c + unit(rng) * rng.uniform(0, 0.002)
        out.append((A, B2.astype(F), g))
    return out


@functools.lru_cache(maxsize=None)
def concentric_pairs(seed, count=PAIRS_PER_CLASS):
    """Nearly concentric round hulls: 16-vertex cylinders and sphere samplings of 3 cm radius, centres at most 4 mm apart."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        def one():
            return (cylinder16(0.03, 0.03) if rng.randint(2) else sphere16(0.03, rng)) @ rot(rng).T
        A, B = one(), one() + unit(rng) * rng.uniform(0, 0.004)
        A, B = A.astype(F), B.astype(F)
        out.append((A, B, (A.astype(np.float64).mean(0) - B.astype(np.float64).mean(0)).astype(F)))
    return out


def oracle_guess(A, B):
    """The guess of orc_eval_gjk, restated in float32: both centroids by repeated c = c + v * (1 / n), then ca - cb."""
    def centroid(V):
        c = np.zeros(3, F)
        inv = F(1.0) / F(len(V))
        for v in np.asarray(V, F):
            c = (c + v * inv).astype(F)
        return c
    return (centroid(A) - centroid(B)).astype(F)


def gjk_arrays(pairs, max_dist=1e9, use_gc=0, gc=None, pair_id=0):
    """The argument arrays of c_gjk_epa for a list of (A, B, guess)."""
    n = len(pairs)
    VA, nA = pack_hulls([p[0] for p in pairs])
    VB, nB = pack_hulls([p[1] for p in pairs])
    guess = np.stack([p[2] for p in pairs]).astype(F)
    md = np.broadcast_to(np.asarray(max_dist, F), (n,)).copy()
    gcs = np.zeros((n, 8), np.int32) if gc is None else np.asarray(gc, np.int32).reshape(n, 8)
    return (VA, nA, VB, nB, guess, md, np.broadcast_to(np.asarray(pair_id, np.int32), (n,)).copy(),
            np.broadcast_to(np.asarray(use_gc, np.int32), (n,)).copy(), gcs)


# ------------------------------------------------------------------------------------------------- man_add, tangents --
@functools.lru_cache(maxsize=None)
def plane_space_cases():
    rng = np.random.RandomState(300)
    ns = [np.array(a, np.float64) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    z0 = F(0.70710678)
    for z in (np.nextafter(z0, F(0)), z0, np.nextafter(z0, F(1)), np.nextafter(np.nextafter(z0, F(1)), F(1))):
        for sg in (1.0, -1.0):
            th = rng.uniform(0, 2 * np.pi)
            r = np.sqrt(1.0 - float(z) ** 2)
            ns.append(np.array([r * np.cos(th), r * np.sin(th), sg * float(z)]))
    ns += [unit(rng) for _ in range(200)]
    return np.asarray(ns, F)                                    # (the z of the threshold cases is a float32 already)


# DevMan as words (rv_dev_collide.h): n, col[4], la[4][3], lb[4][3], nrm[4][3], dist[4], ln[4], lt1[4], lt2[4], acc, age, gc[8]
MAN = dict(n=0, col=1, la=5, lb=17, nrm=29, dist=41, ln=45, lt1=49, lt2=53, acc=57, age=58, gc=59, words=67)
MAN_BREAKING = 0.004


@functools.lru_cache(maxsize=None)
def man_add_cases():
    """(manifolds [n, 67] uint32, points [n, 11] float32 (la, lb, nrm, dist, breaking), colliders [n] int32, tags [n]).
    Every word of a manifold is set, the slots past its n too (man_add loads all four)."""
    rng = np.random.RandomState(400)
    mans, pts, cols, tags = [], [], [], []
    kinds = ['near_same', 'near_other', 'far', 'deeper_than_all', 'deepest0', 'deepest1', 'deepest2', 'deepest3', 'breaking0', 'breaking0_far']
    for rep in range(40):
        for kind in kinds:
            n = 4 if kind.startswith('deep') else rng.randint(0, 5)
            if kind in ('near_same', 'near_other', 'breaking0') and n == 0:
                n = rng.randint(1, 5)
            m = np.zeros(MAN['words'], np.uint32)
            f = m.view(F)
            m.view(np.int32)[MAN['n']] = n
            m.view(np.int32)[MAN['col']:MAN['col'] + 4] = rng.randint(0, 3, 4)
            # anchor points at least 8 mm apart: two candidates never compete for "nearest within breaking"
            while True:
                la = rng.randn(4, 3) * 0.03
                if min(np.linalg.norm(la[i] - la[j]) for i in range(4) for j in range(i)) > 0.008:
                    break
            f[MAN['la']:MAN['la'] + 12] = la.ravel()
            f[MAN['lb']:MAN['lb'] + 12] = rng.randn(12) * 0.03
            f[MAN['nrm']:MAN['nrm'] + 12] = rng.randn(12)
            dist = -rng.permutation(4) * 0.001 - rng.uniform(0.0002, 0.0008, 4)      # 1 mm apart, all different
            f[MAN['ln']:MAN['ln'] + 12] = rng.uniform(0.1, 2.0, 12)                   # impulses: never zero
            f[MAN['acc']] = rng.uniform(0, 0.01)
            m.view(np.int32)[MAN['age']] = rng.randint(0, 100)
            m.view(np.int32)[MAN['gc']:MAN['gc'] + 8] = rng.randint(0, 16, 8)
            pd = rng.uniform(-0.0045, 0.001)
            breaking = MAN_BREAKING
            col = int(rng.randint(0, 3))
            p = rng.randn(3) * 0.03 + unit(rng) * 0.1                                 # far from every anchor
            if kind in ('near_same', 'near_other', 'breaking0'):
                k = rng.randint(0, n)
                p = la[k] + unit(rng) * rng.uniform(0, 0.3) * MAN_BREAKING * (0 if kind == 'breaking0' and rep % 2 else 1)
                col = int(m.view(np.int32)[MAN['col'] + k])
                if kind == 'near_other':
                    col = (col + 1) % 3
                    m.view(np.int32)[MAN['col'] + k] = (col + 2) % 3
            if kind.startswith('breaking0'):
                breaking = 0.0
            if kind == 'deeper_than_all':
                pd = dist.min() - 0.001
            if kind.startswith('deepest'):
                k = int(kind[-1])
                j = int(np.argmin(dist)); dist[[j, k]] = dist[[k, j]]
                pd = dist.min() + 0.0005
            f[MAN['dist']:MAN['dist'] + 4] = dist
            mans.append(m)
            pts.append(np.concatenate([p, rng.randn(3) * 0.03, unit(rng), [pd, breaking]]))
            cols.append(col); tags.append(kind)
    return np.stack(mans), np.asarray(pts, F), np.asarray(cols, np.int32), tags
