"""What saving, branching and look-ahead cost on the device:

    python tools/state_branch_bench.py [--reps 30] [--warmup 5] [--out profiles/state_branch_bench.txt]

At 1024 -> 8192 envs (S = 8) and 64 -> 4096 envs (S = 64), timed with device events, median of `reps` after `warmup`:
  save_state     through the gather kernel and through the runtime's device-to-device copy (RV_STATE_MEMCPY)
  branch_from    against a device-to-device hipMemcpyAsync of the same number of destination bytes, in the same run
  simulate_plans at H = 4 against H plain set_actions + step_macro calls on an ordinary world of N x S envs (put back
                 to its reset state before every repetition, so that its episodes do not run out)
and, not a timing: how many of 64 crossing-layout episodes ShootingPushPolicy and the random policy bring to the goal.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from robovat_amd import configs, lib, scenes

H = 4


def median_ms(fn, reps, warmup, before=None):
    """median device time of fn() in ms: events on the current stream around every repetition"""
    times = []
    for k in range(warmup + reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def world(n, scene, names, **over):
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(**over), n_envs=n, seed=5, shape_names=names)
    return lib.World(cfg, scene, device=0)


def copies(n, s, reps, warmup, say):
    scene, names = scenes.make_scene()
    src, plan, plain = world(n, scene, names), world(n * s, scene, names), world(n * s, scene, names)
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    try:
        src.reset(); plain.reset()
        src.set_actions(src.policy_random(0)); src.step_macro()
        nb = src.state_bytes()
        say('--- %d -> %d envs (S = %d), %d bytes per env block' % (n, n * s, s, nb))
        row = '%-58s median %9.4f ms   min %9.4f   max %9.4f   %s'

        def gbs(nbytes, ms):      # bytes read + bytes written
            return '%7.1f GB/s' % (2.0 * nbytes / (ms * 1e-3) / 1e9)
        for who, w in (('source', src), ('plan-sized world', plain)):
            buf = torch.empty((w.n, nb), dtype=torch.uint8, device=w.device)
            for name, flag in (('gather kernel', '0'), ('runtime copy', '1')):
                os.environ['RV_STATE_MEMCPY'] = flag
                m = median_ms(lambda: lib.check(w.lib.rv_state_save(w.h, w._ptr(buf))), reps, warmup)
                say(row % ('save_state, %s of %d envs, %s' % (who, w.n, name), m[0], m[1], m[2], gbs(w.n * nb, m[0])))
                m = median_ms(lambda: lib.check(w.lib.rv_state_load(w.h, w._ptr(buf), w.n, None)), reps, warmup)
                say(row % ('load_state, %s of %d envs, %s' % (who, w.n, name), m[0], m[1], m[2], gbs(w.n * nb, m[0])))
            os.environ.pop('RV_STATE_MEMCPY')
            m = median_ms(lambda: w.save_state(), reps, warmup)
            say(row % ('save_state() as shipped (with the allocation), %d envs' % w.n, m[0], m[1], m[2], gbs(w.n * nb, m[0])))
        m = median_ms(lambda: plan.branch_from(src, s), reps, warmup)
        say(row % ('branch_from %d -> %d' % (n, n * s), m[0], m[1], m[2], gbs(n * s * nb, m[0])))
        a = torch.empty((n * s, nb), dtype=torch.uint8, device=src.device)
        b = torch.empty((n * s, nb), dtype=torch.uint8, device=src.device)
        m = median_ms(lambda: hip.hipMemcpyAsync(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), n * s * nb, 3, stream), reps, warmup)
        say(row % ('hipMemcpyAsync device-to-device of %d blocks' % (n * s), m[0], m[1], m[2], gbs(n * s * nb, m[0])))
        # look-ahead: branch + H steps + records against H plain steps of a world of the same size
        acts = torch.rand((n, s, H, src.G, 4), device=src.device) * 2.0 - 1.0
        m_plan = median_ms(lambda: plan.plan_simulate(src, acts), reps, warmup)
        say(row % ('simulate_plans, H = %d, %d branch envs' % (H, n * s), m_plan[0], m_plan[1], m_plan[2], ''))
        start = plain.save_state()
        flat = acts.permute(2, 0, 1, 3, 4).reshape(H, n * s, src.G, 4).contiguous()

        def steps():
            for t in range(H):
                plain.set_actions(flat[t]); plain.step_macro()
        m_plain = median_ms(steps, reps, warmup, before=lambda: plain.load_state(start))
        say(row % ('%d x (set_actions + step_macro), ordinary world of %d' % (H, n * s), m_plain[0], m_plain[1], m_plain[2], ''))
        say('simulate_plans / plain stepping = %.3f (the two worlds hold different envs: S copies of %d states / %d reset states)'
            % (m_plan[0] / m_plain[0], n, n * s))
    finally:
        for w in (src, plan, plain):
            w.close()


def success_rate(say, n=64, s=64, h=2, max_steps=8):
    from robovat_amd import policies
    from robovat_amd.envs.push.push_env import VecPushEnv
    cfg = configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0, MAX_STEPS=max_steps)
    out = {}
    for name in ('shooting', 'random'):
        env = VecPushEnv(n, config=cfg, seed=5)
        try:
            env.reset()
            policy = policies.ShootingPushPolicy(env, s, h, gamma=0.9, seed=1) if name == 'shooting' else policies.RandomPolicy(env)
            wins = done_eps = 0
            for _ in range(max_steps):
                env.step(policy.action(None))
                st = env.stats()
                wins += st['successes']; done_eps += st['episodes_done']
            out[name] = (wins, done_eps, float(env.world.episode_returns().mean()))
        finally:
            env.close()
    say('--- crossing layout 0, %d envs, one episode each of at most %d steps; ShootingPushPolicy S = %d, H = %d, gamma 0.9' % (n, max_steps, s, h))
    for name, (wins, eps, ret) in out.items():
        say('%-9s policy: %d of %d episodes reached the goal (%.1f %%), %d episodes ended, mean episode return %.2f'
            % (name, wins, n, 100.0 * wins / n, eps, ret))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-rate', action='store_true')
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    say('tools/state_branch_bench.py --reps %d --warmup %d on %s' % (args.reps, args.warmup, torch.cuda.get_device_name(0)))
    copies(1024, 8, args.reps, args.warmup, say)
    copies(64, 64, args.reps, args.warmup, say)
    if not args.skip_rate:
        success_rate(say)


if __name__ == '__main__':
    main()
