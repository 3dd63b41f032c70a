"""tests/push_proposals_host.py -- the float32 NumPy restatement of csrc/rv_dev_push_sampler.h -- against the C oracle's
policy_heuristic, against the reference's own HeuristicPushSampler.sample (tests/golden/push_proposals_golden.json, written
by gen_push_proposals_golden.py), and against the properties the planning form promises.  No GPU."""
import json
import os

import numpy as np
import pytest

import push_proposals_host as host
from robovat_amd import configs, scenes
from robovat_amd.envs.push.heuristic_push_sampler import HeuristicPushSampler

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 17
SPACE = host.Space([0.35, -0.35], [0.85, 0.35], 0.2, 0.2)
POS = np.array([[0.55, -0.1], [0.7, 0.15], [0.45, 0.2], [0.62, -0.22]], F)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'push_proposals_golden.json')) as f:
        return json.load(f)


def test_episode_mode_with_one_sample_is_the_oracles_policy_heuristic():
    """after reset, after two steps and across an episode end, on an oracle world of 4 envs"""
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(MAX_STEPS=3), n_envs=4, seed=SEED, env_id_offset=5, shape_names=names)
    ref = orc.OracleWorld(cfg, scene, double=False)
    space = host.Space.of(cfg)
    ref.reset()

    def check(moment, max_attempts=2000):
        pos, nb, n_ep, n_st = host.world_inputs(ref.observe(full=True))
        want = ref.policy_heuristic(max_attempts)
        got, status = host.proposals(pos, nb, n_ep, n_st, SEED, 5, space, 1, mode=host.EPISODE, max_attempts=max_attempts)
        assert np.array_equal(_bits(got[:, 0]), _bits(want[:, 0])), moment
        return want, n_ep, n_st

    a, n_ep, n_st = check('after reset')
    assert np.all(n_st == 0)
    for _ in range(2):
        ref.set_actions(a); ref.step_macro()
        a = ref.policy_heuristic(2000)
    a, _, n_st = check('after two steps')
    assert np.any(n_st >= 1)
    ref.set_actions(a); ref.step_macro()
    done = ref.reward()[1].astype(np.uint8)
    assert done.any()
    ref.reset(done)
    _, n_ep2, n_st = check('across an episode end')
    assert np.array_equal(n_ep2, n_ep + done) and np.all(n_st[done != 0] == 0)
    # a budget too small to find anything: the last attempt as drawn, as the oracle returns it
    pos, nb, n_ep, n_st = host.world_inputs(ref.observe(full=True))
    got, status = host.proposals(pos, nb, n_ep, n_st, SEED, 5, space, 1, mode=host.EPISODE, max_attempts=3)
    assert np.array_equal(_bits(got[:, 0]), _bits(ref.policy_heuristic(3)[:, 0])) and np.any(status == host.EXHAUSTED)


def _motion_bound(n_ep):
    """see test_restatement_equals_the_reference_on_the_golden_cases"""
    q = np.floor(42.0 * n_ep / (2.0 * np.pi))
    two_pi_f = float(F(2.0) * host.PI)
    assert np.floor(float(F(42.0 * n_ep)) / two_pi_f) == q      # the float32 reduction takes the same number of turns
    e_base = q * abs(two_pi_f - 2.0 * np.pi) + 0.5 * float(np.spacing(F(two_pi_f * q)))
    e_sum = 0.5 * float(np.spacing(F(4.0)))
    e_sincos = 2.0 * float(np.spacing(F(1.0)))
    e_ref_cast = 0.5 * float(np.spacing(F(1.0)))
    e_noise_sum = float(np.spacing(F(1.0)))
    return e_base + e_sum + e_sincos + e_ref_cast + e_noise_sum


def test_restatement_equals_the_reference_on_the_golden_cases(golden):
    """The reference's sample() was fed the restatement's own uniforms.  Equal: the attempt every candidate took and its
    status.  Bit-equal: the start components (they are the fed draws).  The motion components cos / sin(angle) + noise,
    clipped, agree within a bound derived here, not tuned.  With theta* the reference's float64 angle and theta the
    restatement's float32 one (both use the same fed delta and noise):
      (a) the float32 reduction of 42 n_ep mod 2 pi: 42 n_ep is exact; q turns of the float32 2 pi are off by
          q |2pi_f - 2pi| (q <= 20 at n_ep <= 3: 3.5e-6), the product 2pi_f q is rounded once (half an ulp of a number below
          128: 3.8e-6), and the subtraction of two floats that close is exact;
      (b) one rounded sum base + delta, below 8: half an ulp of [4, 8), 2.4e-7;
      (c) |cos theta - cos theta*| <= |theta - theta*| = (a) + (b), likewise sin;
      (d) sincosr's contract, 2 ulp of a true value of at most 1: 2 x 2^-23;
      (e) the reference rounds its float64 cosine to float32: half an ulp of 1;
      (f) both sides then round value + noise once (the sum is below 2): two half ulps of [1, 2); clipping widens nothing.
    At n_ep = 3 the sum is 8.0e-6."""
    assert _motion_bound(3) < 8.2e-6
    space = host.Space(golden['cspace_low'], golden['cspace_high'], golden['translation_x'], golden['translation_y'])
    seen_nb, seen_s, seen_ep, exhausted_then_found = set(), set(), set(), False
    for c in golden['cases']:
        pos = np.array(c['position'], F).reshape(4, 2)
        want = np.array(c['actions'], F).reshape(c['num_samples'], 4)
        got, status, taken = host.episode(pos, c['nb'], c['num_episodes'], c['num_steps'], c['gid'], golden['world_seed'], space,
                                          c['num_samples'], c['max_attempts'], c['start_margin'], c['motion_margin'])
        assert taken.tolist() == c['taken'] and status.tolist() == c['status']
        assert np.array_equal(_bits(got[:, :2]), _bits(want[:, :2]))
        err = float(np.abs(got[:, 2:].astype(np.float64) - want[:, 2:].astype(np.float64)).max())
        assert err <= _motion_bound(c['num_episodes']), (c['num_episodes'], err)
        seen_nb.add(c['nb']); seen_s.add(c['num_samples']); seen_ep.add(c['num_episodes'])
        st = np.array(c['status'])
        assert st[-1] == host.FOUND
        exhausted_then_found |= bool(np.any((st[:-1] == host.EXHAUSTED) & (st[1:] == host.FOUND)))
    assert seen_nb == {1, 2, 3, 4} and seen_s == {1, 3, 8} and seen_ep == {0, 1, 2, 3} and exhausted_then_found


def _waypoints(a, space=SPACE):
    """start and end of an action, the float32 arithmetic of the header"""
    x = a[..., 0] * (F(0.5) * (space.hi0 - space.lo0)) + F(0.5) * (space.hi0 + space.lo0)
    y = a[..., 1] * (F(0.5) * (space.hi1 - space.lo1)) + F(0.5) * (space.hi1 + space.lo1)
    ex = host.fclampr(x + a[..., 2] * space.tx, space.lo0, space.hi0)
    ey = host.fclampr(y + a[..., 3] * space.ty, space.lo1, space.hi1)
    return x, y, ex, ey


def _d(p, x, y):
    dx, dy = p[0] - x, p[1] - y
    return np.sqrt(dx * dx + dy * dy)


@pytest.mark.parametrize('nb', [1, 3, 4])
def test_spread_candidates_are_safe_and_reach_their_own_body(nb):
    s, copies = 5, 2
    pos = np.stack([POS, POS[::-1]])
    got, status = host.proposals(pos, [nb, nb], [0, 0], [0, 0], SEED, 4, SPACE, s, plan_index=3, step=1, copies=copies, seed=9,
                                 max_attempts=20000)
    assert np.all(status == host.FOUND)
    for m in range(2):
        for k in range(s):
            kg = (m % copies) * s + k
            x, y, ex, ey = _waypoints(got[m, k])
            assert all(_d(pos[m, b], x, y) > F(0.05) for b in range(nb))
            t = pos[m, kg % nb]
            assert not (_d(t, x, y) >= F(0.01) and _d(t, ex, ey) >= F(0.01))
            assert np.all(np.abs(got[m, k]) <= 1.0)


def test_no_two_candidates_share_a_philox_block():
    words = set()
    count = 0
    for gid in (0, 1, 7):
        for plan_index in (0, 1, (1 << 24) - 1):
            for seed in (0, 5):
                c1, c2, c3 = host.spread_key(gid, plan_index, seed)
                assert c3 >> 24 == host.RV_STREAM_PUSH_PROPOSAL and c3 >> 24 not in (1, 2, 3, 4, 5, 7, 8, 9)
                for step in (0, 1, 63):
                    for kg in (0, 1, 2, 1023):
                        first = host.spread_counters(step, kg, np.array([0, 1, 2, 32767], np.uint64))
                        for c0 in first.tolist():
                            for block in (0, 1):
                                assert (c0 + block) < (1 << 32)
                                words.add((c0 + block, c1, c2, c3)); count += 1
    assert len(words) == count
    # the fields of c0 do not overlap: step, candidate and attempt are read back from the word
    c0 = int(host.spread_counters(63, 1023, np.array([32767], np.uint64))[0]) + 1
    assert (c0 >> 26, (c0 >> 16) & 1023, (c0 & 0xffff) >> 1, c0 & 1) == (63, 1023, 32767, 1)
    # and the episode stream is k_policy_heuristic's: stream word 3, c0 = 2 * attempt
    assert host.episode_counters([0, 5]).tolist() == [0, 10] and host.RV_STREAM_HEUR == 3


def test_spread_draws_do_not_depend_on_the_batch_the_split_or_the_copies():
    nb, n0 = [4, 3, 2, 4], [0, 0, 0, 0]
    pos = np.stack([POS, POS * F(0.98), POS[::-1], POS * F(1.02)])
    kw = dict(plan_index=11, step=2, seed=123, max_attempts=4000)
    whole, st_whole = host.proposals(pos, nb, n0, n0, SEED, 0, SPACE, 6, **kw)
    # a shard of two envs at offset 2
    part, st_part = host.proposals(pos[2:], nb[2:], n0[2:], n0[2:], SEED, 2, SPACE, 6, **kw)
    assert np.array_equal(_bits(part), _bits(whole[2:])) and np.array_equal(st_part, st_whole[2:])
    # fewer candidates: a prefix
    few, _ = host.proposals(pos, nb, n0, n0, SEED, 0, SPACE, 2, **kw)
    assert np.array_equal(_bits(few), _bits(whole[:, :2]))
    # three copies of every env, two candidates each: the same six
    rep = np.repeat(pos, 3, axis=0)
    rn = np.repeat(nb, 3)
    z = np.zeros(12, np.int64)
    copied, st_copied = host.proposals(rep, rn, z, z, SEED, 0, SPACE, 2, copies=3, **kw)
    assert np.array_equal(_bits(copied.reshape(4, 6, 4)), _bits(whole)) and np.array_equal(st_copied.reshape(4, 6), st_whole)
    # another plan_index, step or seed: other draws
    for other in (dict(kw, plan_index=12), dict(kw, step=3), dict(kw, seed=124)):
        assert not np.array_equal(host.proposals(pos, nb, n0, n0, SEED, 0, SPACE, 6, **other)[0], whole)


def test_spread_angles_cover_the_circle():
    n = 1 << 16
    ang = []
    for gid in range(n // 1024):
        u = host.spread_u01(SEED, gid, 4, 0, 0, np.arange(1024), 0)      # attempt 0 of every candidate
        ang.append(host.uniform(u[:, 2], -host.PI, host.PI))
    ang = np.concatenate(ang).astype(np.float64)
    assert ang.size == n and ang.min() >= -np.pi - 1e-6 and ang.max() <= np.pi + 1e-6
    quadrant = np.floor(ang / (np.pi / 2)).astype(int).clip(-2, 1)
    assert set(quadrant.tolist()) == {-2, -1, 0, 1}
    assert abs(ang.mean()) < 5.0 / np.sqrt(n)


def _episode_by_hand(pos, nb, n_ep, n_st, gid, s, max_attempts, **margins):
    """the reference's loop, one attempt at a time"""
    out, status, taken, a = [], [], [], -1
    for _ in range(s):
        found = False
        for _ in range(max_attempts):
            a += 1
            r = host.attempt(host.episode_u01(SEED, gid, n_ep, n_st, [a]), False, host.base_angle(n_ep), pos, nb, n_ep % nb, SPACE,
                             margins.get('start_margin', 0.05), margins.get('motion_margin', 0.01))
            if r['good'][0]:
                found = True
                break
        out.append(r['actions'][0]); status.append(int(found)); taken.append(a)
    return np.array(out, F), status, taken


@pytest.mark.parametrize('max_attempts', [1, 2, 100])
def test_episode_budget(max_attempts):
    """One body and a motion margin chosen so that found and exhausted candidates mix at each budget: 20 cm makes about
    every third attempt good (budgets 1 and 2), 3.3 cm about every hundredth (budget 100, where a success then often
    falls into the partial second round of 64).  The candidate after an exhausted one starts at the next attempt."""
    s = 40 if max_attempts < 100 else 24
    margins = dict(start_margin=0.05, motion_margin=0.2 if max_attempts < 100 else 0.033)
    got, status, taken = host.episode(POS, 1, 1, 2, 9, SEED, SPACE, s, max_attempts, **margins)
    want, want_status, want_taken = _episode_by_hand(POS, 1, 1, 2, 9, s, max_attempts, **margins)
    assert taken.tolist() == want_taken and status.tolist() == want_status
    assert np.array_equal(_bits(got), _bits(want))
    assert set(status.tolist()) == {host.FOUND, host.EXHAUSTED}
    used = np.diff(np.concatenate([[-1], taken]))
    assert np.all(used[status == host.EXHAUSTED] == max_attempts) and np.all((used >= 1) & (used <= max_attempts))
    if max_attempts == 100:
        assert np.any((status == host.FOUND) & (used > 64))      # found in the partial second round of its budget


def test_host_sampler_stacks_num_samples():
    sampler = HeuristicPushSampler([0.35, -0.35, 0.02], [0.85, 0.35, 0.02], 0.2, 0.2)
    pos, mask = np.concatenate([POS, np.zeros((4, 1), F)], axis=1).astype(np.float64), np.array([1.0, 1.0, 1.0, 0.0])
    np.random.seed(3)
    three = sampler.sample(pos, mask, 2, 0, num_samples=3)
    np.random.seed(3)
    one = sampler.sample(pos, mask, 2, 0, num_samples=1)
    assert three.shape == (3, 4) and one.shape == (1, 4) and three.dtype == np.float32
    assert np.array_equal(three[0], one[0]) and not np.array_equal(three[1], three[0])
