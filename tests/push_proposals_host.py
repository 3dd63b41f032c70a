"""NumPy restatement of csrc/rv_dev_push_sampler.h (rv_policy_heuristic_multi, both modes), for the tests: float32,
operation for operation, every product and sum rounded on its own.  Inputs are what the kernels read of a world: the
observed positions [M, RV_MAXB, 2], nb / n_ep / n_st per env, the global env ids, the config's cspace and translation and
the params.  sincosr comes from tests/cem_host.py, the Philox block from tests/antipodal_host.py."""
import numpy as np

from antipodal_host import philox
from cem_host import sincosr, fclampr

F = np.float32
RV_STREAM_HEUR = 3
RV_STREAM_PUSH_PROPOSAL = 6
RV_HP_MAX_SAMPLES, RV_HP_MAX_ATTEMPTS = 1024, 32768
EPISODE, SPREAD = 0, 1
FOUND, EXHAUSTED = 1, 0
TWO_M24 = F(5.9604644775390625e-8)
PI = F(3.14159265358979323846)
CHUNK = 4096


class Space(object):
    """the config words an attempt reads: cspace_low / cspace_high [0 .. 1], translation_x / _y, as float32"""

    def __init__(self, low, high, translation_x, translation_y):
        self.lo0, self.lo1, self.hi0, self.hi1 = F(low[0]), F(low[1]), F(high[0]), F(high[1])
        self.tx, self.ty = F(translation_x), F(translation_y)

    @classmethod
    def of(cls, cfg):
        """from an rv_config"""
        return cls(list(cfg.cspace_low), list(cfg.cspace_high), cfg.translation_x, cfg.translation_y)


def world_inputs(obs):
    """what the kernels read of every env, from an observation (lib.World.observe() or OracleWorld.observe(full=True)):
    (pos float32 [M, RV_MAXB, 2], nb, n_ep, n_st int [M]) -- nb counts the movable bodies, 1 standing in for 0"""
    get = lambda k: obs[k].cpu().numpy() if hasattr(obs[k], 'cpu') else np.asarray(obs[k])      # noqa: E731
    pos = np.ascontiguousarray(get('position')[..., :2].astype(F))
    nb = np.maximum(get('body_mask').astype(np.int64).sum(axis=1), 1)
    return pos, nb, get('num_episodes').astype(np.int64), get('num_steps').astype(np.int64)


def _u01(words):
    return (np.asarray(words, np.uint64) >> np.uint64(8)).astype(F) * TWO_M24


def _five(c0, c1, c2, c3, world_seed):
    """the five u01 of the attempts whose first block has counter word c0 (an array): block c0 and one word of c0 + 1"""
    c0 = np.asarray(c0, np.uint64)
    full = [np.full_like(c0, int(v) & 0xFFFFFFFF) for v in (c1, c2, c3)]
    a = philox(c0, full[0], full[1], full[2], world_seed & 0xFFFFFFFF, world_seed >> 32)
    b = philox(c0 + np.uint64(1), full[0], full[1], full[2], world_seed & 0xFFFFFFFF, world_seed >> 32)
    return np.stack([_u01(a[0]), _u01(a[1]), _u01(a[2]), _u01(a[3]), _u01(b[0])], axis=-1)


def episode_counters(attempts):
    """c0 of the first block of EPISODE attempts"""
    return np.asarray(attempts, np.uint64) * np.uint64(2)


def spread_counters(step, kg, attempts):
    """c0 of the first block of SPREAD attempts of candidate kg at plan step `step` (kg and attempts broadcast)"""
    kg, a = np.broadcast_arrays(np.asarray(kg, np.uint64), np.asarray(attempts, np.uint64))
    assert 0 <= step < 64 and (kg.size == 0 or (int(kg.max()) < 1024 and int(a.max()) < (1 << 15)))
    return (np.uint64(step) << np.uint64(26)) | (kg << np.uint64(16)) | (a * np.uint64(2))


def spread_key(gid, plan_index, seed):
    """(c1, c2, c3) of a SPREAD draw"""
    assert 0 <= plan_index < (1 << 24)
    return int(seed) & 0xFFFFFFFF, int(gid), (RV_STREAM_PUSH_PROPOSAL << 24) | int(plan_index)


def episode_u01(world_seed, gid, n_ep, n_st, attempts):
    """the five u01 of EPISODE attempts (k_policy_heuristic's stream) -> float32 [len(attempts), 5]"""
    return _five(episode_counters(attempts), n_ep * 64 + n_st, gid, RV_STREAM_HEUR, world_seed)


def spread_u01(world_seed, gid, plan_index, step, seed, kg, attempts):
    """the five u01 of SPREAD attempts of candidate kg -> float32 [len(attempts), 5]"""
    c1, c2, c3 = spread_key(gid, plan_index, seed)
    return _five(spread_counters(step, kg, attempts), c1, c2, c3, world_seed)


def uniform(u, lo, hi):
    """rng_uniform: lo + (hi - lo) * u01, the bounds float32 expressions as the header writes them"""
    lo, hi = F(lo), F(hi)
    return lo + (hi - lo) * u


def base_angle(n_ep):
    base = F(n_ep) * F(42.0)
    two_pi = F(2.0) * PI
    return base - two_pi * np.floor(base / two_pi)


def _dist(px, py, x, y):
    dx, dy = px - x, py - y
    return np.sqrt(dx * dx + dy * dy)


def attempt(u, spread, base, pos, nb, target, space, start_margin, motion_margin):
    """hp_attempt over a batch: u float32 [A, 5]; pos [RV_MAXB, 2]; -> dict: actions [A, 4], good / safe / effective [A],
    start_dist [A, nb] (to every body), target_dist [A, 2] (start and end to the target)"""
    pos = np.asarray(pos, F)
    s0, s1 = uniform(u[:, 0], -1.0, 1.0), uniform(u[:, 1], -1.0, 1.0)
    if spread:
        ang = uniform(u[:, 2], -PI, PI)
    else:
        ang = F(base) + uniform(u[:, 2], F(-0.25) * PI, F(0.25) * PI)
    sn, co = sincosr(ang)
    m0 = fclampr(co + uniform(u[:, 3], -0.3, 0.3), -1.0, 1.0)
    m1 = fclampr(sn + uniform(u[:, 4], -0.3, 0.3), -1.0, 1.0)
    sp = space
    x = s0 * (F(0.5) * (sp.hi0 - sp.lo0)) + F(0.5) * (sp.hi0 + sp.lo0)
    y = s1 * (F(0.5) * (sp.hi1 - sp.lo1)) + F(0.5) * (sp.hi1 + sp.lo1)
    ex = fclampr(x + m0 * sp.tx, sp.lo0, sp.hi0)
    ey = fclampr(y + m1 * sp.ty, sp.lo1, sp.hi1)
    sd = np.stack([_dist(pos[b, 0], pos[b, 1], x, y) for b in range(nb)], axis=-1)
    safe = np.all(sd > F(start_margin), axis=-1)
    d1, d2 = _dist(pos[target, 0], pos[target, 1], x, y), _dist(pos[target, 0], pos[target, 1], ex, ey)
    clear = (d1 >= F(motion_margin)) & (d2 >= F(motion_margin))
    return {'actions': np.stack([s0, s1, m0, m1], axis=-1).astype(F), 'good': safe & ~clear, 'safe': safe, 'effective': ~clear,
            'start_dist': sd.astype(F), 'target_dist': np.stack([d1, d2], axis=-1).astype(F)}


def episode(pos, nb, n_ep, n_st, gid, world_seed, space, s, max_attempts, start_margin=0.05, motion_margin=0.01, trace=None):
    """RV_HP_EPISODE for one env -> (actions float32 [s, 4], status int32 [s], attempt int64 [s]: the attempt each
    candidate took, in the env's one sequence).  ``trace``: a list that receives attempt()'s dict of every chunk scanned."""
    nb = max(int(nb), 1)
    target, base = int(n_ep) % nb, base_angle(n_ep)
    cache = {}

    def chunk(i):
        if i not in cache:
            at = np.arange(i * CHUNK, (i + 1) * CHUNK, dtype=np.uint64)
            cache[i] = attempt(episode_u01(world_seed, gid, n_ep, n_st, at), False, base, pos, nb, target, space, start_margin, motion_margin)
            if trace is not None:
                trace.append((i * CHUNK, cache[i]))
        return cache[i]

    actions, status, taken = np.zeros((s, 4), F), np.zeros(s, np.int32), np.zeros(s, np.int64)
    cursor = 0
    for k in range(s):
        end, a, found = cursor + max_attempts, cursor, False      # the budget: attempts [cursor, end)
        while a < end:
            i = a // CHUNK
            good = chunk(i)['good']
            hi = min(end, (i + 1) * CHUNK)
            hit = np.flatnonzero(good[a - i * CHUNK:hi - i * CHUNK])
            if hit.size:
                a, found = a + int(hit[0]), True
                break
            a = hi
        if not found:
            a = end - 1      # the last attempt of the budget, as drawn
        actions[k] = chunk(a // CHUNK)['actions'][a % CHUNK]
        status[k], taken[k] = (FOUND if found else EXHAUSTED), a
        cursor = a + 1
    return actions, status, taken


def spread_candidate(pos, nb, gid, world_seed, space, kg, plan_index, step, seed, max_attempts, start_margin=0.05, motion_margin=0.01):
    """one RV_HP_SPREAD candidate -> (action float32 [4], status, attempt)"""
    nb = max(int(nb), 1)
    target = int(kg) % nb
    for lo in range(0, max_attempts, CHUNK):
        at = np.arange(lo, min(lo + CHUNK, max_attempts), dtype=np.uint64)
        r = attempt(spread_u01(world_seed, gid, plan_index, step, seed, kg, at), True, 0.0, pos, nb, target, space, start_margin, motion_margin)
        hit = np.flatnonzero(r['good'])
        if hit.size:
            return r['actions'][hit[0]], FOUND, lo + int(hit[0])
    return r['actions'][-1], EXHAUSTED, max_attempts - 1


def proposals(pos, nb, n_ep, n_st, world_seed, env_id_offset, space, s, mode=SPREAD, plan_index=0, step=0, copies=1, seed=0,
              max_attempts=20000, start_margin=0.05, motion_margin=0.01):
    """rv_policy_heuristic_multi on a world of M envs: pos [M, RV_MAXB, 2], nb / n_ep / n_st [M] -> (actions float32
    [M, s, 4] -- one goal step's worth; the kernel repeats it G times --, status int32 [M, s])"""
    pos = np.asarray(pos, F)
    M = pos.shape[0]
    assert 1 <= s <= RV_HP_MAX_SAMPLES and copies >= 1 and copies * s <= RV_HP_MAX_SAMPLES and 1 <= max_attempts <= RV_HP_MAX_ATTEMPTS
    assert env_id_offset % copies == 0
    actions, status = np.zeros((M, s, 4), F), np.zeros((M, s), np.int32)
    for m in range(M):
        if mode == EPISODE:
            assert plan_index == 0 and step == 0 and seed == 0 and copies == 1
            actions[m], status[m], _ = episode(pos[m], nb[m], int(n_ep[m]), int(n_st[m]), env_id_offset + m, world_seed, space, s,
                                               max_attempts, start_margin, motion_margin)
        else:
            gid, copy = (env_id_offset + m) // copies, m % copies
            for k in range(s):
                actions[m, k], status[m, k], _ = spread_candidate(pos[m], nb[m], gid, world_seed, space, copy * s + k, plan_index, step,
                                                                  seed, max_attempts, start_margin, motion_margin)
    return actions, status
