"""Generate tests/golden/push_proposals_golden.json by RUNNING the reference's HeuristicPushSampler.sample(position,
body_mask, num_episodes, num_steps, num_samples) (build container only).

    python tests/golden/gen_push_proposals_golden.py

gen_golden.py is imported for the stubs it installs and for the reference module.  ``np.random.uniform`` is replaced, while
the reference runs, by a feeder that hands out the uniforms tests/push_proposals_host.py draws in RV_HP_EPISODE mode, in
call order (per attempt: the start [2], the angle, the motion noise [2]), so that the reference and the restatement consume
the same randomness.  Only DATA is written: the inputs, the attempts each candidate took, the reference's actions and the
statuses.

The reference decides in float64 and the restatement in float32: a case with any scanned attempt whose start distance (to
any body) or end distance (to the target) lies within MARGIN_GAP of either margin would test rounding, not the sampler.
Such a case is not written: the global env id -- a Philox key word -- is advanced until the case is clean and its last
candidate is found.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden  # noqa: E402  (the stubs; gen_golden.hps is the reference module)

import push_proposals_host as host  # noqa: E402

F = np.float32
WORLD_SEED = 7 + (5 << 32)
LOW, HIGH, TX, TY = [0.35, -0.35], [0.85, 0.35], 0.2, 0.2      # PUSH_ENV_CONFIG's ACTION.CSPACE / MOTION
MARGIN_GAP = 1e-4
MAX_TRIES = 200000
CASES = [
    # nb, num_samples, num_episodes, num_steps, start_margin, motion_margin, max_attemps, first gid, an exhausted candidate?
    (1, 8, 0, 0, 0.05, 0.01, 20000, 100, False),
    (2, 3, 1, 2, 0.05, 0.01, 20000, 200, False),
    (3, 3, 2, 1, 0.05, 0.01, 20000, 300, False),
    (4, 1, 3, 0, 0.05, 0.01, 20000, 400, False),
    (4, 8, 1, 3, 0.05, 0.03, 20000, 500, False),
    (2, 1, 0, 1, 0.05, 0.01, 20000, 600, False),
    (3, 8, 3, 2, 0.05, 0.03, 20000, 700, False),
    # a budget so small that a candidate runs out while the next one still succeeds
    (3, 3, 2, 0, 0.05, 0.01, 600, 800, True),
]


def f32_list(a):
    """float32 values as the shortest decimals that read back to the same float32"""
    return [float(str(v)) for v in np.asarray(a, F).reshape(-1)]


def positions(rng, nb):
    """nb bodies inside the cspace, 12 cm apart at least; absent rows zero, as PoseObs gives them"""
    pos = np.zeros((4, 2), F)
    k = 0
    while k < nb:
        p = rng.uniform([LOW[0] + 0.08, LOW[1] + 0.08], [HIGH[0] - 0.08, HIGH[1] - 0.08])
        if all(np.hypot(*(p - pos[j])) > 0.12 for j in range(k)):
            pos[k] = p
            k += 1
    return pos


def clean(trace, taken, start_margin, motion_margin):
    """no scanned attempt (those up to the last one taken) next to a margin"""
    last = int(taken[-1])
    for first, r in trace:
        n = min(len(r['good']), last + 1 - first)
        if n <= 0:
            continue
        d = np.concatenate([r['start_dist'][:n].reshape(-1), r['target_dist'][:n, 1]]).astype(np.float64)
        for margin in (start_margin, motion_margin):
            if np.any(np.abs(d - margin) < MARGIN_GAP):
                return False
    return True


def main():
    rng = np.random.RandomState(20261019)
    space = host.Space(LOW, HIGH, TX, TY)
    cases = []
    for nb, s, n_ep, n_st, start_margin, motion_margin, max_att, gid0, want_exhausted in CASES:
        pos = positions(rng, nb)
        for gid in range(gid0, gid0 + MAX_TRIES):
            trace = []
            actions, status, taken = host.episode(pos, nb, n_ep, n_st, gid, WORLD_SEED, space, s, max_att, start_margin, motion_margin, trace)
            if status[-1] != host.FOUND:      # every case reaches its last candidate
                continue
            if want_exhausted != bool(np.any((status[:-1] == host.EXHAUSTED) & (status[1:] == host.FOUND))):
                continue
            if not want_exhausted and not np.all(status == host.FOUND):
                continue
            if clean(trace, taken, start_margin, motion_margin):
                break
        else:
            raise SystemExit('no clean case found for %r' % ((nb, s, n_ep, n_st),))
        # the restatement's uniforms of attempts 0 .. taken[-1], in the reference's call order
        n_att = int(taken[-1]) + 1
        u = host.episode_u01(WORLD_SEED, gid, n_ep, n_st, np.arange(n_att, dtype=np.uint64))
        pi = host.PI
        feed = {'i': 0, 'call': 0}
        bounds = [(F(-1.0), F(1.0), 2, (0, 1)), (F(-0.25) * pi, F(0.25) * pi, None, (2,)), (F(-0.3), F(0.3), 2, (3, 4))]

        def uniform(low=0.0, high=1.0, size=None):
            lo, hi, n, cols = bounds[feed['call']]
            assert abs(low - float(lo)) < 1e-6 and abs(high - float(hi)) < 1e-6 and (size is None) == (n is None) and (size is None or list(size) == [n])
            vals = [float(host.uniform(u[feed['i'], c], lo, hi)) for c in cols]
            feed['call'] += 1
            if feed['call'] == 3:
                feed['call'], feed['i'] = 0, feed['i'] + 1
            return vals[0] if size is None else np.array(vals, np.float64)

        sampler = gen_golden.hps.HeuristicPushSampler(
            cspace_low=[float(F(v)) for v in LOW] + [0.02], cspace_high=[float(F(v)) for v in HIGH] + [0.02],
            translation_x=float(F(TX)), translation_y=float(F(TY)),
            start_margin=float(F(start_margin)), motion_margin=float(F(motion_margin)), max_attemps=max_att)
        pos3 = np.concatenate([pos.astype(np.float64), np.zeros((4, 1))], axis=1)
        mask = (np.arange(4) < nb).astype(np.float64)
        keep = np.random.uniform
        np.random.uniform = uniform
        try:
            ref = sampler.sample(pos3, mask, n_ep, n_st, s)
        finally:
            np.random.uniform = keep
        assert ref.shape == (s, 4) and ref.dtype == F
        assert feed['i'] == n_att and feed['call'] == 0, 'the reference scanned %d attempts, the restatement %d' % (feed['i'], n_att)
        # the attempt each of the reference's pushes came from: the one whose fed start it carries
        fed = np.stack([host.uniform(u[:, 0], -1.0, 1.0), host.uniform(u[:, 1], -1.0, 1.0)], axis=-1)
        ref_taken = []
        for k in range(s):
            at = np.flatnonzero((fed[:, 0] == ref[k, 0]) & (fed[:, 1] == ref[k, 1]))
            assert at.size == 1, 'a start that is not one fed attempt'
            ref_taken.append(int(at[0]))
        # its status, from how many attempts the call consumed: fewer than the budget means found
        used = np.diff([-1] + ref_taken)
        assert np.all(used >= 1) and np.all(used <= max_att) and np.all(used[status == host.EXHAUSTED] == max_att)
        assert np.all(status[used < max_att] == host.FOUND)
        taken = ref_taken
        cases.append({
            'nb': nb, 'num_samples': s, 'num_episodes': n_ep, 'num_steps': n_st, 'gid': gid,
            'start_margin': start_margin, 'motion_margin': motion_margin, 'max_attempts': max_att,
            'position': f32_list(pos), 'taken': [int(v) for v in taken], 'status': [int(v) for v in status],
            'actions': f32_list(ref),
        })
        print('case nb=%d S=%d n_ep=%d: gid %d, attempts taken %s, status %s' % (nb, s, n_ep, gid, list(taken), list(status)))
    with open(os.path.join(HERE, 'push_proposals_golden.json'), 'w') as f:
        json.dump({'world_seed': WORLD_SEED, 'cspace_low': LOW, 'cspace_high': HIGH, 'translation_x': TX, 'translation_y': TY,
                   'margin_gap': MARGIN_GAP, 'cases': cases}, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
