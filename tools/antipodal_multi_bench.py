"""Time rv_policy_antipodal_multi and try_grasps, and measure what one step of look-ahead buys GraspReward.

    python tools/antipodal_multi_bench.py [--n 2048 --ks 1,8,16 --try-k 8 --policy-ks 4,8 --steps 3]

Three measurements on config-4 envs (Grasp4DofEnv), all on one device and in one process:
  kernel   rv_policy_antipodal (one grasp) and rv_policy_antipodal_multi at each K of --ks on the same rendered depth
           images, timed alternately with device events (warm-up first, then the median of --iters calls each; a call
           is the binding plus one launch).  The kernels alone: run this under rocprofv3 --kernel-trace --stats.
  try      try_grasps of --try-k candidates per env (branch to N x K copies, one env.step() of the copies, rewards)
           against --try-k plain steps of the N envs themselves (set_actions, step_macro, reward; and again as whole
           env.step() calls, which add the depth observation), each restored to the same state first (the restore is
           outside the timed region).
  success  GraspReward success rate of LookaheadGrasp4DofPolicy at each K of --policy-ks against
           AntipodalGrasp4DofPolicy, on envs of the same seed, --steps episodes each.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robovat_amd import envs, lib, policies  # noqa: E402


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def stat(v):
    return 'median %.3f ms  (min %.3f, max %.3f, %d calls)' % (float(np.median(v)), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2048); ap.add_argument('--seed', type=int, default=9)
    ap.add_argument('--ks', default='1,8,16'); ap.add_argument('--try-k', type=int, default=8)
    ap.add_argument('--policy-ks', default='4,8'); ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3); ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('antipodal_multi_bench: no GPU (a timing needs the device)')
    ks = [int(k) for k in a.ks.split(',') if k]
    policy_ks = [int(k) for k in a.policy_ks.split(',') if k]
    out = {'n': a.n, 'seed': a.seed}

    # -- kernel
    env = envs.VecGrasp4DofEnv(a.n, seed=a.seed)
    env.reset()
    world = env.world
    depth, _ = world.render(segmask=False)
    params = lib.antipodal_params()
    runs = [('one grasp', lambda: world.policy_antipodal(params, 0, depth=depth))]
    for k in ks:
        runs.append(('multi K=%d' % k, lambda k=k: world.policy_antipodal_multi(params, 0, k, depth=depth)))
    for _ in range(a.warmup):
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in runs}
    for _ in range(a.iters):      # alternately, so that all see the same machine
        for name, fn in runs:
            times[name].append(timed(torch, fn))
    print('rv_policy_antipodal_multi against rv_policy_antipodal: %d config-4 envs, the same depth images' % a.n)
    for name, _ in runs:
        print('  %-12s %s' % (name, stat(times[name])))
    g, _, cnt, st = world.policy_antipodal_multi(params, 0, max(ks), depth=depth)
    cnt = cnt.cpu().numpy()
    print('  grasps found at K=%d: mean %.2f, envs with none %d, envs with all %d' % (max(ks), cnt.mean(), int((cnt == 0).sum()), int((cnt == max(ks)).sum())))
    out['kernel_ms'] = {name: float(np.median(v)) for name, v in times.items()}
    out['mean_count'] = float(cnt.mean())

    # -- try_grasps
    K = a.try_k
    if K > 0:
        env.sample_antipodal_candidates(K)
        a4 = env.antipodal_actions4
        snap = env.save_state()
        for _ in range(a.warmup):
            env.try_grasps(a4)
            env.world.set_actions(a4[:, 0]); env.world.step_macro(); env.world.reward()
            env.restore_state(snap)
        torch.cuda.synchronize()
        t_try, t_steps, t_env = [], [], []
        for _ in range(max(a.iters // 4, 3)):
            t_try.append(timed(torch, lambda: env.try_grasps(a4)))
            total = 0.0
            for k in range(K):
                env.restore_state(snap)

                def one(k=k):
                    env.world.set_actions(a4[:, k]); env.world.step_macro(); env.world.reward()
                total += timed(torch, one)
            t_steps.append(total)
            total = 0.0
            for k in range(K):
                env.restore_state(snap)
                total += timed(torch, lambda k=k: env.step(a4[:, k]))
            t_env.append(total)
            env.restore_state(snap)
        print('try_grasps: %d envs x %d candidates' % (a.n, K))
        print('  try_grasps (branch + one step of %d copies + rewards): %s' % (a.n * K, stat(t_try)))
        print('  %d plain steps of the %d envs (set_actions, step_macro, reward):    %s' % (K, a.n, stat(t_steps)))
        print('  %d env.step() calls (the same plus the depth observation and its calibration): %s' % (K, stat(t_env)))
        print('  plain steps / try_grasps: %.2fx; env.step() calls / try_grasps: %.2fx' %
              (float(np.median(t_steps)) / float(np.median(t_try)), float(np.median(t_env)) / float(np.median(t_try))))
        out['try_grasps_ms'] = float(np.median(t_try)); out['plain_steps_ms'] = float(np.median(t_steps)); out['env_steps_ms'] = float(np.median(t_env))
    env.close()

    # -- success rate
    def success(make_policy):
        env = envs.VecGrasp4DofEnv(a.n, seed=a.seed)
        policy = make_policy(env)
        rates = []
        for _ in range(a.steps):
            obs = env.reset()
            _, r, _, _ = env.step(policy.action(obs))
            rates.append(float((r > 0).float().mean()))
        env.close()
        return rates
    if a.steps > 0:
        base = success(lambda e: policies.AntipodalGrasp4DofPolicy(e))
        print('GraspReward success rate, %d envs, seed %d, %d episodes each' % (a.n, a.seed, a.steps))
        print('  AntipodalGrasp4DofPolicy (one grasp):  %s  mean %.3f' % (' '.join('%.3f' % v for v in base), np.mean(base)))
        out['success'] = {'one': float(np.mean(base))}
        for k in policy_ks:
            rates = success(lambda e, k=k: policies.LookaheadGrasp4DofPolicy(e, k))
            print('  LookaheadGrasp4DofPolicy K=%-2d:          %s  mean %.3f' % (k, ' '.join('%.3f' % v for v in rates), np.mean(rates)))
            out['success']['K%d' % k] = float(np.mean(rates))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
