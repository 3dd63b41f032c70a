"""NumPy restatement of the contact-record builder of rv_get_contact_points (robovat_amd/csrc/rv_dev_contacts.h),
read from the CPU oracle's world: PyBullet's getContactPoints records (bullet_physics.py:1262-1304) of one env.

The oracle's manifold accessor does not return the collider index of an arm point, so the link of an arm record is
found by geometry: the link frame f whose collider boxes hold lb (lb is a local point of frame f, on the surface of the
collider, pushed out by the margin), best first by how well positionOnB then sits where the point's distance and normal
say it is.  Where several frames pass (the restatement cannot tell them apart) every record carries the alternatives."""
import numpy as np

from robovat_amd import abi

ARM_CODE = abi.RV_CP_ARM
BB_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
assert len(BB_PAIRS) == abi.RV_NBB


def qmat(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def plane_space(n):
    """rv_dev_collide.h plane_space: the solver's two friction directions of normal n."""
    n = np.asarray(n, np.float64)
    if abs(n[2]) > 0.7071067811865476:
        a = n[1] ** 2 + n[2] ** 2
        k = 1.0 / np.sqrt(a)
        t1 = np.array([0.0, -n[2] * k, n[1] * k])
        t2 = np.array([a * k, -n[0] * t1[2], n[0] * t1[1]])
    else:
        a = n[0] ** 2 + n[1] ** 2
        k = 1.0 / np.sqrt(a)
        t1 = np.array([-n[1] * k, n[0] * k, 0.0])
        t2 = np.array([-n[2] * t1[1], n[2] * t1[0], a * k])
    return t1, t2


def man_owner(mi):
    """(kind, a, b) of manifold slot mi: 0 body-table, 1 body-body, 2 arm-body."""
    if mi < abi.RV_MAXB:
        return 0, mi, -1
    if mi < abi.RV_MAXB + abi.RV_NBB:
        a, b = BB_PAIRS[mi - abi.RV_MAXB]
        return 1, a, b
    return 2, mi - abi.RV_MAXB - abi.RV_NBB, -1


def arm_links(arm, links, lb, wa, nrm, dist, margin):
    """The link frames an arm point may ride on, best first (see the module docstring)."""
    col_frame = list(arm.col_frame)
    found = []
    for f in sorted(set(col_frame)):
        inside = False
        for col in range(abi.RV_NCOL):
            if col_frame[col] != f:
                continue
            c = np.array(list(arm.col_center[col])); h = np.array(list(arm.col_half[col]))
            inside |= bool(np.all(np.abs(lb - c) <= h + margin + 2e-3))
        if not inside:
            continue
        wb = links[f, :3] + qmat(links[f, 3:7]) @ lb
        found.append((float(np.linalg.norm(wa - wb - dist * nrm)), f))
    return [f for _, f in sorted(found)]


def side_match(qb, ql, body, link):
    return (qb < 0 or qb == body) and (ql < 0 or link < 0 or link == ql)


def records(world, scene, cfg, env, query=(-1, -1, -1, -1)):
    """([(ids[4], data[RV_CP_NF], alts), ...], count) of one env of an orc.OracleWorld, in the device's order.  alts:
    for an arm point, {link: (ids, data)} of every link frame it may ride on (ids / data are the best one's); else None."""
    qa, qla, qb, qlb = query
    bs = world.body_state()[env]
    links = world.link_poses()[env]
    flags = world.query_contacts()[env]
    counts = world.manifold_counts()[env]
    dt = float(np.float32(cfg.dt))
    cand = []
    for mi in range(abi.RV_NMAN):
        kind, a, b = man_owner(mi)
        n, pts = world.manifold(env, mi)
        assert n == counts[mi]
        for i in range(n):
            la, lb, nrm = pts[i, 0:3], pts[i, 3:6], pts[i, 6:9]
            dist, ln, lt1, lt2 = pts[i, 9:13]
            if kind == 2 and not (flags[2 + a] and np.float32(dist) < np.float32(cfg.contact_query_dist)):
                continue
            wa = bs[a, :3] + qmat(bs[a, 3:7]) @ la
            if kind == 0:
                B, lkb, wb = abi.RV_CP_TABLE, -1, lb.copy()
            elif kind == 1:
                B, lkb, wb = b, -1, bs[b, :3] + qmat(bs[b, 3:7]) @ lb
            else:
                fs = arm_links(scene.arm, links, lb, wa, nrm, dist, float(cfg.margin))
                assert fs, (env, mi, i)
                cand.append([[a, abi.RV_CP_ARM, -1, f, wa, links[f, :3] + qmat(links[f, 3:7]) @ lb, nrm.copy(), dist,
                              ln / dt, lt1 / dt, lt2 / dt] for f in fs])
                continue
            cand.append([[a, B, -1, lkb, wa, wb, nrm.copy(), dist, ln / dt, lt1 / dt, lt2 / dt]])
    if flags[0]:
        nan3 = np.full(3, np.nan)
        cand.append([[abi.RV_CP_ARM, abi.RV_CP_TABLE, -1, -1, nan3, nan3, np.array([0.0, 0.0, 1.0]), np.nan, 0.0, 0.0, 0.0]])
    out = []
    for alts in cand:
        kept = {}
        for A, B, lka, lkb, pa, pb, n, dist, fn, f1, f2 in alts:
            d1, d2 = plane_space(n)
            swap = (B == qa and A != qa) if qa >= 0 else (qb >= 0 and A == qb and B != qb)
            if swap:
                A, B, lka, lkb, pa, pb, n, d1, d2 = B, A, lkb, lka, pb, pa, -n, -d1, -d2
            if side_match(qa, qla, A, lka) and side_match(qb, qlb, B, lkb):
                data = np.concatenate([pa, pb, n, [dist, fn, f1], d1, [f2], d2])
                kept[max(lka, lkb)] = (np.array([A, B, lka, lkb], np.int32), data)
        if kept:
            first = next(iter(kept.values()))
            out.append((first[0], first[1], kept if ARM_CODE in (first[0][0], first[0][1]) and max(kept) >= 0 else None))
    return out, len(out)


def net_force(recs):
    """fn n + f1 d1 + f2 d2 summed over records: the contact force on body A."""
    f = np.zeros(3)
    for r in recs:
        d = r[1]
        f += d[10] * d[6:9] + d[11] * d[12:15] + d[15] * d[16:19]
    return f


def old_hit(flags, counts, a, b):
    """The hit test HipPhysics.get_contact_points answered before the records existed, for a pair (a, b) of body codes
    (slots, RV_CP_TABLE, RV_CP_ARM), either order."""
    if b == abi.RV_CP_ARM and a != abi.RV_CP_ARM:
        a, b = b, a
    if a == abi.RV_CP_TABLE and b < abi.RV_MAXB:
        a, b = b, a
    if a == abi.RV_CP_ARM:
        if b == abi.RV_CP_TABLE:
            return bool(flags[0])
        return 0 <= b < abi.RV_MAXB and bool(flags[2 + b])
    if a < abi.RV_MAXB:
        if b == abi.RV_CP_TABLE:
            return bool(counts[a] > 0)
        for k, (x, y) in enumerate(BB_PAIRS):
            if {a, b} == {x, y} and counts[abi.RV_MAXB + k] > 0:
                return True
    return False
