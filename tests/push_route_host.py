"""NumPy restatement of csrc/rv_dev_push_route.h (rv_get_route_field / rv_policy_route_multi), for the tests: float32,
operation for operation, every product and sum rounded on its own.  The route field is built by a plain queue BFS from
the goal cells -- another algorithm than the kernel's relaxation.  Inputs are what the kernels read: the rv_config's
tiles, cspace and translation, the observed positions [M, RV_MAXB, 2], the movable-body count and whether body 0 is
movable, the global env ids and the params.  The Philox block, rng_uniform, sincosr and fclampr are those of
tests/push_proposals_host.py."""
import collections

import numpy as np

from push_proposals_host import F, FOUND, EXHAUSTED, Space, _u01, uniform, philox, sincosr, fclampr

RV_STREAM_PUSH_ROUTE = 10
RV_TASK_INSERTION, RV_TASK_CROSSING = 2, 3
GRID, CELLS, NONE = 8, 64, 255
INF = F(np.inf)
DEFAULTS = dict(plan_index=0, step=0, copies=1, max_attempts=256, seed=0, keep_nominal=1, start_margin=0.05, angle_jitter=0.3,
                back_lo=0.08, back_hi=0.16, lateral=0.02, length_lo=0.8, length_hi=1.2)


def params(**over):
    assert set(over) <= set(DEFAULTS), sorted(set(over) - set(DEFAULTS))
    return dict(DEFAULTS, **over)


def tiles(cfg):
    """(task, region cells, goal cells) of an rv_config; a cell is r * 8 + c"""
    def cells(lst, n):
        out = []
        for j in range(n):
            r, c = float(lst[j][0]), float(lst[j][1])
            assert r == int(r) and c == int(c) and 0 <= r < GRID and 0 <= c < GRID
            out.append(int(r) * GRID + int(c))
        return out
    return int(cfg.task), cells(cfg.region, cfg.n_region), cells(cfg.goal, cfg.n_goal)


# synthetic tile lists (region, goal) for crossing worlds.  WRAP: (0, 7) and (1, 0) are lanes 7 and 8 of the kernel's wave
# and no neighbours; (1, 0) reaches the goal (1, 1), (0, 7) nothing.  ISLAND: (0, 0) and (0, 1) are walkable but cut off
# from the goal (3, 4), which (3, 3) reaches
WRAP = ([(0, 7), (1, 0)], [(1, 1)])
ISLAND = ([(0, 0), (0, 1), (3, 3)], [(3, 4)])


def set_tiles(cfg, region, goal, task=RV_TASK_CROSSING):
    """give an rv_config (ctypes) other tiles, in place"""
    cfg.task, cfg.n_region, cfg.n_goal = task, len(region), len(goal)
    for lst, cells in ((cfg.region, region), (cfg.goal, goal)):
        for j, t in enumerate(cells):
            lst[j][0], lst[j][1] = float(t[0]), float(t[1])
    return cfg


def walkable(cfg):
    task, region, goal = tiles(cfg)
    assert task in (RV_TASK_CROSSING, RV_TASK_INSERTION) and goal
    w = np.zeros(CELLS, bool) if task == RV_TASK_CROSSING else np.ones(CELLS, bool)
    w[region] = task == RV_TASK_CROSSING
    w[goal] = True
    return w


def neighbours(i):
    """the 4-neighbours of cell i in the grid, in the header's order: (r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)"""
    r, c = divmod(i, GRID)
    return [rr * GRID + cc for rr, cc in ((r + 1, c), (r - 1, c), (r, c + 1), (r, c - 1)) if 0 <= rr < GRID and 0 <= cc < GRID]


def route_field(cfg):
    """D uint8 [64]: hops through walkable cells to the nearest goal cell; 255 = not walkable or no goal reached"""
    walk = walkable(cfg)
    d = np.full(CELLS, NONE, np.uint8)
    queue = collections.deque()
    for g in tiles(cfg)[2]:
        if d[g] != 0:
            d[g] = 0
            queue.append(g)
    while queue:
        i = queue.popleft()
        for j in neighbours(i):
            if walk[j] and d[j] == NONE:
                d[j] = d[i] + 1
                queue.append(j)
    return d


class Route(object):
    """what the proposal kernel reads besides the env: D, walkable, the cell centres, cspace and translation"""

    def __init__(self, cfg):
        self.d, self.walk = route_field(cfg), walkable(cfg)
        size, off0, off1 = F(cfg.tile_size), F(cfg.tile_offset[0]), F(cfg.tile_offset[1])
        idx = np.arange(CELLS)
        self.cx = off0 + (idx // GRID).astype(F) * size
        self.cy = off1 + (idx % GRID).astype(F) * size
        self.space = Space.of(cfg)

    def _argmin(self, q, among):
        key = np.where(among & (q < INF), q, INF)      # (a NaN is not below +inf)
        return int(np.flatnonzero(among & (key == key.min()))[0])

    def aim(self, px, py):
        """(cur, aim cell) for body 0 at (px, py)"""
        qx, qy = self.cx - F(px), self.cy - F(py)
        q = qx * qx + qy * qy
        cur = self._argmin(q, self.walk)
        if self.d[cur] == 0:
            return cur, cur
        if self.d[cur] == NONE:
            return cur, self._argmin(q, self.d == 0)
        return cur, [j for j in neighbours(cur) if self.d[j] == self.d[cur] - 1][0]

    def direction(self, px, py):
        """(ux, uy, dist, cur, aim cell)"""
        px, py = F(px), F(py)
        cur, a = self.aim(px, py)
        vx, vy = self.cx[a] - px, self.cy[a] - py
        dist = np.sqrt(vx * vx + vy * vy)
        if dist > F(1e-6):
            return vx / dist, vy / dist, dist, cur, a
        return F(1.0), F(0.0), dist, cur, a


def route_u01(world_seed, gid, plan_index, step, seed, kg, attempts):
    """the four u01 of attempts of candidate kg -> float32 [len(attempts), 4]"""
    a = np.asarray(attempts, np.uint64)
    assert 0 <= step < 64 and 0 <= kg < 1024 and 0 <= plan_index < (1 << 24) and (a.size == 0 or int(a.max()) < (1 << 15))
    c0 = (np.uint64(step) << np.uint64(26)) | (np.uint64(kg) << np.uint64(16)) | a
    c1, c2, c3 = int(seed) & 0xFFFFFFFF, int(gid), (RV_STREAM_PUSH_ROUTE << 24) | int(plan_index)
    o = philox(c0, np.full_like(c0, c1), np.full_like(c0, c2), np.full_like(c0, c3), world_seed & 0xFFFFFFFF, world_seed >> 32)
    return np.stack([_u01(w) for w in o], axis=-1)


def attempt(route, pos, nb, ux, uy, dist, jit, back, lat, f, start_margin):
    """pr_attempt over a batch: jit / back / lat / f float32 [A]; pos [RV_MAXB, 2] -> dict: actions [A, 4], good [A],
    start [A, 2] (world), direction [A, 2], start_dist [A, nb]"""
    pos, sp = np.asarray(pos, F), route.space
    px, py = pos[0, 0], pos[0, 1]
    jit, back, lat, f = [np.ascontiguousarray(v, F) for v in (jit, back, lat, f)]
    sn, co = sincosr(jit)
    dx, dy = ux * co - uy * sn, ux * sn + uy * co
    x = fclampr((px - dx * back) - dy * lat, sp.lo0, sp.hi0)
    y = fclampr((py - dy * back) + dx * lat, sp.lo1, sp.hi1)
    ln = (dist + back) * f
    m0 = fclampr(dx * (ln / sp.tx), -1.0, 1.0)
    m1 = fclampr(dy * (ln / sp.ty), -1.0, 1.0)
    s0 = fclampr((x - F(0.5) * (sp.hi0 + sp.lo0)) / (F(0.5) * (sp.hi0 - sp.lo0)), -1.0, 1.0)
    s1 = fclampr((y - F(0.5) * (sp.hi1 + sp.lo1)) / (F(0.5) * (sp.hi1 - sp.lo1)), -1.0, 1.0)
    sd = []
    for b in range(nb):
        ex, ey = pos[b, 0] - x, pos[b, 1] - y
        sd.append(np.sqrt(ex * ex + ey * ey))
    sd = np.stack(sd, axis=-1)
    return {'actions': np.stack([s0, s1, m0, m1], axis=-1).astype(F), 'good': np.all(sd > F(start_margin), axis=-1),
            'start': np.stack([x, y], axis=-1), 'direction': np.stack([dx, dy], axis=-1), 'start_dist': sd.astype(F)}


def candidate(route, pos, nb, movable0, gid, world_seed, kg, p, trace=None):
    """one candidate -> (action float32 [4], status, attempt taken).  ``trace``: a list that receives (direction() of the
    wave, attempt()'s dict) of every chunk scanned"""
    if not movable0:
        return np.zeros(4, F), EXHAUSTED, -1
    nb = max(int(nb), 1)
    pos = np.asarray(pos, F)
    aim = route.direction(pos[0, 0], pos[0, 1])
    ux, uy, dist = aim[:3]
    one = np.ones(1, F)
    if p['keep_nominal'] and kg == 0:
        r = attempt(route, pos, nb, ux, uy, dist, 0 * one, (F(0.5) * (F(p['back_lo']) + F(p['back_hi']))) * one, 0 * one, one, p['start_margin'])
        if trace is not None:
            trace.append((aim, r))
        return r['actions'][0], (FOUND if r['good'][0] else EXHAUSTED), 0
    chunk = 4096
    for lo in range(0, p['max_attempts'], chunk):
        at = np.arange(lo, min(lo + chunk, p['max_attempts']), dtype=np.uint64)
        u = route_u01(world_seed, gid, p['plan_index'], p['step'], p['seed'], kg, at)
        r = attempt(route, pos, nb, ux, uy, dist, uniform(u[:, 0], -F(p['angle_jitter']), F(p['angle_jitter'])),
                    uniform(u[:, 1], p['back_lo'], p['back_hi']), uniform(u[:, 2], -F(p['lateral']), F(p['lateral'])),
                    uniform(u[:, 3], p['length_lo'], p['length_hi']), p['start_margin'])
        if trace is not None:
            trace.append((aim, r))
        hit = np.flatnonzero(r['good'])
        if hit.size:
            return r['actions'][hit[0]], FOUND, lo + int(hit[0])
    return r['actions'][-1], EXHAUSTED, p['max_attempts'] - 1


def world_inputs(obs):
    """what the kernel reads of every env, from an observation (lib.World.observe() or OracleWorld.observe(full=True)):
    (pos float32 [M, RV_MAXB, 2], nb int [M], movable0 bool [M])"""
    get = lambda k: obs[k].cpu().numpy() if hasattr(obs[k], 'cpu') else np.asarray(obs[k])      # noqa: E731
    mask = get('body_mask') != 0
    return np.ascontiguousarray(get('position')[..., :2].astype(F)), np.maximum(mask.sum(axis=1), 1), mask[:, 0]


def proposals(route, pos, nb, movable0, world_seed, env_id_offset, s, p):
    """rv_policy_route_multi on a world of M envs -> (actions float32 [M, s, 4] -- one goal step's worth; the kernel
    repeats it G times --, status int32 [M, s])"""
    pos = np.asarray(pos, F)
    M, copies = pos.shape[0], p['copies']
    assert 1 <= s <= 1024 and copies >= 1 and copies * s <= 1024 and 1 <= p['max_attempts'] <= 32768 and env_id_offset % copies == 0
    actions, status = np.zeros((M, s, 4), F), np.zeros((M, s), np.int32)
    for m in range(M):
        gid, copy = (env_id_offset + m) // copies, m % copies
        for k in range(s):
            actions[m, k], status[m, k], _ = candidate(route, pos[m], nb[m], movable0[m], gid, world_seed, copy * s + k, p)
    return actions, status
