"""The cross-entropy-method planner on the device: what its two kernels cost, and what it buys.

    python tools/cem_bench.py [--iters 30] [--warmup 5] [--out profiles/cem_bench.txt] [--skip-kernels] [--skip-rate]

(a) rv_cem_sample and rv_cem_refit against a plain-torch restatement on the same device -- randn, topk, mean, std as a
    user without the kernels would write them; it is the yardstick, not the code under test, and it draws other numbers
    (torch's generator is a stream, not a key) -- at N = 1024, H = 8, S = 64 and S = 1024, E = S / 8.  Timed alternately
    with device events, warm-up first, the median of --iters calls each; every figure includes the binding's allocations.
    Then the two kernels' share of one CEMPushPolicy.plan() call at the shapes of (b).
(b) DESIGN.md 14's goal-rate experiment: crossing layout 0, 64 envs, one episode each of at most 8 steps, gamma 0.9.
    CEMPushPolicy against ShootingPushPolicy at the SAME number of simulated candidate steps per decision (I x S x H of
    the one = S x H of the other), and against RandomPolicy.  Reported: goal count, episodes ended, mean episode return.
    Not a timing, and no bar is set on it.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch

from robovat_amd import configs, lib, scenes
from benchlib import alternate, make_push_policy, rate_line, run_episodes, BUDGETS, GAMMA


def torch_sample(mean, std, s, gen):
    z = torch.randn((mean.shape[0], s, mean.shape[1]), generator=gen, device=mean.device, dtype=torch.float32)
    x = (mean[:, None] + std[:, None] * z).clamp(-1.0, 1.0)
    x[:, 0] = mean.clamp(-1.0, 1.0)
    return x


def torch_refit(x, returns, mean, std, e, alpha, min_std):
    idx = returns.topk(e, dim=1).indices
    xe = x.gather(1, idx[:, :, None].expand(-1, -1, x.shape[2]))
    m, sd = xe.mean(dim=1), xe.std(dim=1, unbiased=False)
    return alpha * mean + (1.0 - alpha) * m, (alpha * std + (1.0 - alpha) * sd).clamp_min(min_std), idx


def kernels(say, n, s, h, iters, warmup):
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n, seed=5, shape_names=names)
    w = lib.World(cfg, scene, device=0)
    try:
        d, e = h * w.G * 4, max(1, s // 8)
        gen = torch.Generator(device=w.device); gen.manual_seed(1)
        mean = torch.rand((n, d), generator=gen, device=w.device) - 0.5
        std = torch.full((n, d), 0.5, device=w.device)
        returns = torch.randn((n, s), generator=gen, device=w.device)
        p = lib.cem_params(plan_index=0, iteration=0, seed=1, keep_mean=1, n_elites=e, alpha=0.25, min_std=0.05)
        x = w.cem_sample(mean, std, p, s, h)
        flat = x.reshape(n, s, d)
        # the two agree on what they compute: same elites (the returns have no ties), moments within float32 noise
        km, ks, kel = w.cem_refit(x, returns, mean, std, p)
        tm, ts, tel = torch_refit(flat, returns, mean, std, e, 0.25, 0.05)
        torch.cuda.synchronize()
        agree = (float((kel.long() == tel).float().mean()), float((km - tm).abs().max()), float((ks - ts).abs().max()))
        t = alternate({'k_sample': lambda: w.cem_sample(mean, std, p, s, h), 't_sample': lambda: torch_sample(mean, std, s, gen),
                       'k_refit': lambda: w.cem_refit(x, returns, mean, std, p),
                       't_refit': lambda: torch_refit(flat, returns, mean, std, e, 0.25, 0.05)}, iters, warmup)
        say('--- N = %d, S = %d, H = %d (D = %d floats per plan), E = %d; %d calls each after %d warm-up' % (n, s, h, d, e, iters, warmup))
        row = '  %-44s median %8.4f ms   min %8.4f   max %8.4f'
        say(row % (('rv_cem_sample (one launch, incl. the binding)',) + t['k_sample']))
        say(row % (('torch: randn, multiply-add, clamp, row 0',) + t['t_sample']))
        say(row % (('rv_cem_refit (one launch, incl. the binding)',) + t['k_refit']))
        say(row % (('torch: topk, gather, mean, std, smoothing',) + t['t_refit']))
        say('  torch / kernel: sample %.1fx, refit %.1fx;  candidates written %.1f MB -> %.2f TB/s; elites read twice %.1f MB'
            % (t['t_sample'][0] / t['k_sample'][0], t['t_refit'][0] / t['k_refit'][0], n * s * d * 4 / 1e6,
               n * s * d * 4 / (t['k_sample'][0] * 1e-3) / 1e12, 2 * n * e * d * 4 / 1e6))
        say('  agreement of the refit with the restatement: elites equal %.4f %%, largest |mean| difference %.3g, |std| %.3g'
            % (100.0 * agree[0], agree[1], agree[2]))
    finally:
        w.close()


def share(say, budget, iters, warmup, n=64):
    """the two kernels' part of one plan() call"""
    from robovat_amd.envs.push.push_env import VecPushEnv
    it, s, h = budget
    env = VecPushEnv(n, config=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), seed=5)
    try:
        env.reset()
        policy = make_push_policy('cem', env, budget, GAMMA)
        mean = policy.initial_mean()
        std = torch.full_like(mean, 0.5)
        cand = env.sample_plan_candidates(mean, std, s, 0, 1)
        returns = torch.randn((n, s), device=env.device)

        def plan():
            policy.reset(); policy.plan()
        t = alternate({'plan': plan, 'sample': lambda: env.sample_plan_candidates(mean, std, s, 0, 1),
                       'refit': lambda: env.refit_plan_distribution(cand, returns, mean, std, policy.num_elites, 0.0, 0.05)}, iters, warmup)
        part = it * (t['sample'][0] + t['refit'][0])
        say('--- one CEMPushPolicy.plan() call, %d envs, I = %d, S = %d, H = %d, E = %d: median %.2f ms; its %d x (sample %.4f ms + '
            'refit %.4f ms) = %.3f ms are %.2f %% of it (the rest: %d macro launches of the env kernel on %d branch envs, and scoring)'
            % (n, it, s, h, policy.num_elites, t['plan'][0], it, t['sample'][0], t['refit'][0], part, 100.0 * part / t['plan'][0], it * h, n * s))
    finally:
        env.close()


def goal_rate(say, budget, n=64, max_steps=8):
    it, s, h = budget
    cfg = configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0, MAX_STEPS=max_steps)
    say('--- crossing layout 0, %d envs, one episode each of at most %d steps, gamma %.1f; %d simulated candidate steps per decision:'
        ' CEMPushPolicy I = %d, S = %d, H = %d (defaults otherwise: E = %d, init_std 0.5, min_std 0.05, alpha 0, warm start) against'
        ' ShootingPushPolicy S = %d, H = %d' % (n, max_steps, GAMMA, it * s * h, it, s, h, max(1, s // 8), it * s, h))
    for name in ('cem', 'shooting', 'random'):
        c = run_episodes(name, cfg, budget, GAMMA, n, max_steps)
        say(rate_line(name, c, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-kernels', action='store_true')
    ap.add_argument('--skip-rate', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('cem_bench: no GPU (a timing needs the device)')
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    say('tools/cem_bench.py --iters %d --warmup %d on %s' % (args.iters, args.warmup, torch.cuda.get_device_name(0)))
    if not args.skip_kernels:
        for s in (64, 1024):
            kernels(say, 1024, s, 8, args.iters, args.warmup)
        share(say, BUDGETS[0], max(3, args.iters // 6), 1)
    if not args.skip_rate:
        for budget in BUDGETS:
            goal_rate(say, budget)


if __name__ == '__main__':
    main()
