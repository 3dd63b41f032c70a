"""tests/push_route_host.py -- the float32 NumPy restatement of csrc/rv_dev_push_route.h -- against hand-checked route
fields, the properties the proposals promise, and end to end on the C oracle: the nominal push alone has to reach the
goal.  No GPU."""
import numpy as np
import pytest

import push_route_host as host
from robovat_amd import configs, scenes

F = np.float32
SEED = 5
LAYOUTS = [(task, layout) for task in ('crossing', 'insertion') for layout in range(3)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(task='crossing', layout=0, n=4, offset=0, seed=SEED, max_steps=8):
    scene, names = scenes.make_scene()
    env_cfg = configs.push_env_config(TASK_NAME=task, LAYOUT_ID=layout, MAX_STEPS=max_steps)
    return configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, env_id_offset=offset, shape_names=names), scene


def wrap_config():
    return host.set_tiles(_cfg()[0], *host.WRAP)


def island_config():
    return host.set_tiles(_cfg()[0], *host.ISLAND)


def _slow_field(cfg):
    """hops to the goal by repeated relaxation over python sets (as the prototype did it)"""
    walk = host.walkable(cfg)
    goal = set(host.tiles(cfg)[2])
    d = {i: (0 if i in goal else 10 ** 6) for i in range(64) if walk[i]}
    for _ in range(64):
        for i in d:
            for j in host.neighbours(i):
                if j in d and d[j] + 1 < d[i]:
                    d[i] = d[j] + 1
    return np.array([d[i] if i in d and d[i] < 10 ** 6 else 255 for i in range(64)], np.uint8)


@pytest.mark.parametrize('task,layout', LAYOUTS)
def test_bfs_field_on_the_layouts(task, layout):
    cfg, _ = _cfg(task, layout)
    d = host.route_field(cfg)
    walk = host.walkable(cfg)
    _, region, goal = host.tiles(cfg)
    assert np.array_equal(d, _slow_field(cfg))
    assert all(d[g] == 0 for g in goal) and np.all(d[~walk] == 255)
    assert np.all(walk[goal])
    if task == 'crossing':
        assert walk.sum() == len(set(region) | set(goal))
    else:
        assert walk.sum() == 64 - len(set(region) - set(goal))
    # every reached cell off the goal has a neighbour one hop closer, and none closer than that
    for i in np.flatnonzero((d != 255) & (d != 0)):
        assert min(int(d[j]) for j in host.neighbours(i)) == int(d[i]) - 1


def test_field_of_crossing_layout_0_by_hand():
    d = host.route_field(_cfg('crossing', 0)[0]).reshape(8, 8)
    assert d[2, 5] == 4 and d[1, 2] == 0
    assert (d[0, 0], d[1, 0], d[1, 1], d[1, 2]) == (3, 2, 1, 0)
    assert d[0, 1] == 255      # (0, 0) has (1, 0) as its only way on
    assert np.all(d[4:] == 255) and np.all(d[:, 6:] == 255)


def test_row_ends_are_no_neighbours():
    d = host.route_field(wrap_config()).reshape(8, 8)
    assert d[1, 1] == 0 and d[1, 0] == 1 and d[0, 7] == 255
    assert 8 not in host.neighbours(7) and 7 not in host.neighbours(8)


def test_island_aims_at_the_goal_centre():
    cfg = island_config()
    r = host.Route(cfg)
    d = r.d.reshape(8, 8)
    assert d[0, 0] == 255 and d[0, 1] == 255 and d[3, 3] == 1 and d[3, 4] == 0
    assert r.walk[0] and r.walk[1]
    px, py = r.cx[0] + F(0.01), r.cy[0] - F(0.02)
    cur, aim = r.aim(px, py)
    assert cur == 0 and aim == 3 * 8 + 4
    ux, uy, dist, _, _ = r.direction(px, py)
    want = np.array([float(r.cx[aim]) - float(px), float(r.cy[aim]) - float(py)])
    assert abs(float(dist) - np.linalg.norm(want)) < 1e-6
    assert np.allclose([ux, uy], want / np.linalg.norm(want), atol=1e-6)


def test_aim_on_the_goal_between_two_cells_and_off_the_tiles():
    r = host.Route(_cfg('crossing', 0)[0])
    goal = 1 * 8 + 2
    assert r.aim(r.cx[goal] + F(0.03), r.cy[goal]) == (goal, goal)
    # exactly midway between (2, 3) and (2, 4): the lower index is the cell, the aim its neighbour towards the goal
    a, b = 2 * 8 + 3, 2 * 8 + 4
    mx, my = r.cx[a], F(0.5) * (r.cy[a] + r.cy[b])
    qa = (r.cx[a] - mx) ** 2 + (r.cy[a] - my) ** 2
    qb = (r.cx[b] - mx) ** 2 + (r.cy[b] - my) ** 2
    assert qa == qb      # (float32: this midpoint is exact)
    assert r.aim(mx, my) == (a, 2 * 8 + 2)
    # a body outside every walkable cell is taken to the nearest one: (7, 7)'s corner of the table -> (2, 5), aim (2, 4)
    assert r.aim(r.cx[63], r.cy[63]) == (2 * 8 + 5, 2 * 8 + 4)
    # the first neighbour in the header's order wins among several one hop closer (none here has two; the order itself:)
    assert host.neighbours(9) == [17, 1, 10, 8]


POS = np.array([[0.62, -0.05], [0.7, 0.15], [0.45, 0.2], [0.66, -0.22]], F)


def test_properties_of_1000_candidates():
    cfg, _ = _cfg('crossing', 0)
    r = host.Route(cfg)
    p = host.params(keep_nominal=0, start_margin=0.09, max_attempts=64, seed=3, plan_index=2, step=1)
    sp = r.space
    ux, uy, dist, cur, aim = r.direction(POS[0, 0], POS[0, 1])
    found = exhausted = 0
    for kg in range(1000):
        trace = []
        a, status, taken = host.candidate(r, POS, 4, True, 7, SEED, kg, p, trace=trace)
        res = trace[-1][1]
        j = taken % 4096
        assert np.array_equal(_bits(a), _bits(res['actions'][j]))
        x, y = res['start'][j]
        assert sp.lo0 <= x <= sp.hi0 and sp.lo1 <= y <= sp.hi1 and np.all(np.abs(a) <= 1.0)
        # the action's start is that point, normalised (float32 division: a few ulp of 1)
        assert abs(float(a[0]) - (float(x) - 0.6) / 0.25) < 2e-6 and abs(float(a[1]) - float(y) / 0.35) < 2e-6
        d64 = np.hypot(POS[:, 0].astype(np.float64) - float(x), POS[:, 1].astype(np.float64) - float(y))
        if status == host.FOUND:
            found += 1
            assert np.all(d64 > 0.09 - 1e-6)
        else:
            exhausted += 1
            assert taken == 63 and np.any(d64 <= 0.09 + 1e-6)
        dx, dy = [float(v) for v in res['direction'][j]]
        # unit length and within the jitter of the aim direction (sincosr: 2 ulp; the products: a few more)
        assert abs(np.hypot(dx, dy) - 1.0) < 1e-5
        assert np.abs(np.arctan2(float(ux) * dy - float(uy) * dx, dx * float(ux) + dy * float(uy))) <= 0.3 + 1e-5
    assert found > 500 and exhausted >= 0


def test_exhaustion_returns_the_last_draw():
    r = host.Route(_cfg('crossing', 0)[0])
    p = host.params(keep_nominal=0, start_margin=0.3, max_attempts=5)      # no start 0.3 clear of body 0 with back <= 0.16
    a, status, taken = host.candidate(r, POS, 4, True, 0, SEED, 3, p)
    assert status == host.EXHAUSTED and taken == 4
    q = host.params(keep_nominal=0, start_margin=0.0, max_attempts=5)
    trace = []
    host.candidate(r, POS, 4, True, 0, SEED, 3, q, trace=trace)
    assert np.array_equal(_bits(a), _bits(trace[0][1]['actions'][4]))
    # body 0 not movable: the zero action
    a, status, _ = host.candidate(r, POS, 3, False, 0, SEED, 3, p)
    assert status == host.EXHAUSTED and not a.any()


def test_nominal_candidate_is_the_closed_form():
    cfg, _ = _cfg('crossing', 0)
    r = host.Route(cfg)
    p = host.params()
    a, status, _ = host.candidate(r, POS, 4, True, 0, SEED, 0, p)
    assert status == host.FOUND
    cur, aim = r.aim(POS[0, 0], POS[0, 1])
    assert (cur, aim) == (2 * 8 + 3, 2 * 8 + 2)
    off, size = np.array(list(cfg.tile_offset), np.float64), float(cfg.tile_size)
    A = off + np.array([2, 2]) * size
    v = A - POS[0].astype(np.float64)
    dist = np.linalg.norm(v)
    u, back = v / dist, 0.5 * (0.08 + 0.16)
    lo, hi = np.array(list(cfg.cspace_low)[:2], np.float64), np.array(list(cfg.cspace_high)[:2], np.float64)
    start = (POS[0] - u * back - 0.5 * (hi + lo)) / (0.5 * (hi - lo))
    motion = u * (dist + back) / np.array([cfg.translation_x, cfg.translation_y])
    assert np.allclose(a, np.concatenate([np.clip(start, -1, 1), np.clip(motion, -1, 1)]), atol=2e-6)
    # candidate 0 without keep_nominal is a drawn one; other candidates never are the nominal
    b, _, _ = host.candidate(r, POS, 4, True, 0, SEED, 0, host.params(keep_nominal=0))
    c, _, _ = host.candidate(r, POS, 4, True, 0, SEED, 1, p)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)


def test_keys_do_not_depend_on_the_batch():
    r = host.Route(_cfg('crossing', 0)[0])
    rng = np.random.RandomState(1)
    pos = np.tile(POS, (6, 1, 1)) + rng.uniform(-0.02, 0.02, (6, 4, 2)).astype(F)
    nb, mov = np.full(6, 4), np.ones(6, bool)
    p = host.params(plan_index=4, step=2, seed=9)
    a, st = host.proposals(r, pos, nb, mov, SEED, 0, 6, p)
    # fewer envs, fewer candidates: the same
    b, stb = host.proposals(r, pos[:2], nb[:2], mov[:2], SEED, 0, 3, p)
    assert np.array_equal(_bits(a[:2, :3]), _bits(b)) and np.array_equal(st[:2, :3], stb)
    # a shard at offset 2
    c, stc = host.proposals(r, pos[2:4], nb[2:4], mov[2:4], SEED, 2, 6, p)
    assert np.array_equal(_bits(a[2:4]), _bits(c)) and np.array_equal(st[2:4], stc)
    # six copies of env 1 with one candidate each (copies = 6, kg = the copy) are env 1's six candidates
    d, std = host.proposals(r, np.tile(pos[1], (6, 1, 1)), nb, mov, SEED, 6, 1, dict(p, copies=6))
    assert np.array_equal(_bits(a[1]), _bits(d[:, 0])) and np.array_equal(st[1], std[:, 0])
    # three copies with two candidates each: kg = copy * 2 + k
    e, ste = host.proposals(r, np.tile(pos[1], (3, 1, 1)), nb[:3], mov[:3], SEED, 3, 2, dict(p, copies=3))
    assert np.array_equal(_bits(a[1]), _bits(e.reshape(6, 4))) and np.array_equal(st[1], ste.reshape(6))
    # and they are six different pushes; another seed, step or plan index gives others
    assert len({tuple(x) for x in a[1].tolist()}) == 6
    for other in (dict(seed=10), dict(step=3), dict(plan_index=5)):
        f, _ = host.proposals(r, pos[:1], nb[:1], mov[:1], SEED, 0, 6, dict(p, **other))
        assert np.array_equal(_bits(a[0, 0]), _bits(f[0, 0])) and not np.array_equal(_bits(a[0, 1:]), _bits(f[0, 1:]))


# the floor: a condition a broken aim cannot meet (policy_heuristic reaches 0 to 2 of 32 on these envs); measured with
# this restatement: see DESIGN.md §19
@pytest.mark.parametrize('task,layout', [('crossing', 0), ('crossing', 1), ('crossing', 2), ('insertion', 0)])
def test_nominal_push_reaches_the_goal_on_the_oracle(task, layout):
    from oracle import orc
    n = 32
    cfg, scene = _cfg(task, layout, n=n, seed=5, max_steps=8)
    w = orc.OracleWorld(cfg, scene, double=False)
    r = host.Route(cfg)
    p = host.params()
    w.reset()
    alive, wins = np.ones(n, bool), np.zeros(n, bool)
    for step in range(8):
        pos, nb, mov = host.world_inputs(w.observe(full=True))
        a, _ = host.proposals(r, pos, nb, mov, 5, 0, 1, dict(p, plan_index=step))
        w.set_actions(np.repeat(a[:, 0][:, None, :], w.G, axis=1))
        w.step_macro()
        rew, done = w.reward()
        wins |= alive & (rew > 50)
        alive &= ~done.astype(bool)
    print('%s layout %d: the nominal push reaches the goal in %d of %d' % (task, layout, int(wins.sum()), n))
    assert int(wins.sum()) >= 12
