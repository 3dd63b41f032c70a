"""What the *_bench.py tools share: the two timers, the push policies of the goal-rate experiments and their episode loop."""
import time

import numpy as np
import torch

GAMMA = 0.9
# (CEM iterations, CEM samples, horizon): shooting and the proposal policies get iterations x samples candidates
BUDGETS = ((4, 16, 2), (4, 32, 4))


def alternate(fns, iters, warmup):
    """median / min / max device ms of every fn, called in turn so that all see the same machine"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = dict((k, []) for k in fns)
    for _ in range(iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            times[name].append(a.elapsed_time(b))
    return dict((k, (float(np.median(v)), float(np.min(v)), float(np.max(v)))) for k, v in times.items())


def wall(fn, reps=3):
    """median wall-clock seconds of ``reps`` synchronised calls after one warm-up call"""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def make_push_policy(name, env, budget, gamma):
    """'route' / 'heuristic' / 'shooting' / 'cem' at the same simulated candidate steps per decision; else RandomPolicy"""
    from robovat_amd import policies
    it, s, h = budget
    if name == 'route':
        return policies.RouteShootingPushPolicy(env, it * s, h, gamma=gamma, seed=1)
    if name == 'heuristic':
        return policies.HeuristicShootingPushPolicy(env, it * s, h, gamma=gamma, seed=1)
    if name == 'cem':
        return policies.CEMPushPolicy(env, s, h, num_iterations=it, gamma=gamma, seed=1)
    if name == 'shooting':
        return policies.ShootingPushPolicy(env, it * s, h, gamma=gamma, seed=1)
    return policies.RandomPolicy(env)


def run_episodes(name, cfg, budget, gamma, n, max_steps, after_step=None):
    """One episode of at most ``max_steps`` steps in each of ``n`` envs (seed 5) under policy ``name``;
    ``after_step(policy)`` is called after every env.step().  Returns the counters summed over the steps (wins,
    done_eps, steps, ineffective, useful) and mean_return."""
    from robovat_amd.envs.push.push_env import VecPushEnv
    env = VecPushEnv(n, config=cfg, seed=5)
    try:
        env.reset()
        policy = make_push_policy(name, env, budget, gamma)
        c = dict(wins=0, done_eps=0, steps=0, ineffective=0, useful=0)
        for _ in range(max_steps):
            env.step(policy.action(None))
            st = env.stats()
            c['wins'] += st['successes']; c['done_eps'] += st['episodes_done']
            c['steps'] += st['env_steps']; c['ineffective'] += st['ineffective']; c['useful'] += st['useful']
            if after_step is not None:
                after_step(policy)
        c['mean_return'] = float(env.world.episode_returns().mean())
        return c
    finally:
        env.close()


def rate_line(name, c, n, extra=None):
    """the line of a goal-rate table for the counters ``c`` of ``run_episodes``; with ``extra`` (a string, '' too) also the
    env steps and their effective and useful shares, then ``extra``"""
    line = ('  %-9s policy: %d of %d episodes reached the goal (%.1f %%), %d episodes ended, mean episode return %.2f'
            % (name, c['wins'], n, 100.0 * c['wins'] / n, c['done_eps'], c['mean_return']))
    if extra is None:
        return line
    return line + ('; %d env steps, effective %.1f %%, useful %.1f %%%s'
                   % (c['steps'], 100.0 * (c['steps'] - c['ineffective']) / max(c['steps'], 1),
                      100.0 * c['useful'] / max(c['steps'], 1), extra))
