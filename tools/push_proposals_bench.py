"""Aimed push proposals for look-ahead: what the sampling kernel costs, and what the proposals buy.

    python tools/push_proposals_bench.py [--iters 30] [--warmup 5] [--out profiles/push_proposals_bench.txt]
                                         [--skip-kernels] [--skip-rate]

(a) rv_policy_heuristic_multi at N = 1024 envs, S = 64 candidates, RV_HP_SPREAD, the reference's margins (0.05 / 0.01),
    against what a user would write in torch on the same device: a FIXED number of attempts (--attempts, 2048) drawn for
    all candidates at once, the margin tests on all of them, the first success taken by an argmax over the flags.  The
    torch code is the yardstick, not the code under test, and it draws other numbers (torch's generator is a stream, not
    a key).  The kernel is timed with the same budget and with the default one (20000).  Timed alternately with device
    events, warm-up first, the median of --iters calls each, min and max alongside; every figure includes the binding's
    allocations.
(b) DESIGN.md 14 / 16's goal-rate experiment: crossing layout 0, 64 envs, seed 5, one episode each of at most 8 steps,
    gamma 0.9.  HeuristicShootingPushPolicy at the simulated candidate steps per decision of section 16's rows (128: S =
    64, H = 2; 512: S = 128, H = 4) next to ShootingPushPolicy, CEMPushPolicy and RandomPolicy, each with its share of
    effective pushes (env steps that stats() does not count as ineffective) and of useful ones (safe and effective).
    Not a timing, and no bar is set on it.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch

from robovat_amd import configs, lib, scenes
from benchlib import alternate, rate_line, run_episodes, BUDGETS, GAMMA


def torch_proposals(pos, mask, s, attempts, cfg, start_margin, motion_margin, gen):
    """pos [N, B, 2], mask [N, B] (1 = a body) -> (actions [N, s, 4], found [N, s]): `attempts` tries per candidate at once"""
    n, nb = pos.shape[0], mask.sum(dim=1).clamp_min(1).long()
    u = torch.rand((5, n, s, attempts), generator=gen, device=pos.device, dtype=torch.float32)
    s0, s1 = u[0] * 2.0 - 1.0, u[1] * 2.0 - 1.0
    ang = (u[2] * 2.0 - 1.0) * math.pi
    m0 = (torch.cos(ang) + (u[3] * 0.6 - 0.3)).clamp(-1.0, 1.0)
    m1 = (torch.sin(ang) + (u[4] * 0.6 - 0.3)).clamp(-1.0, 1.0)
    lo0, hi0, lo1, hi1 = cfg.cspace_low[0], cfg.cspace_high[0], cfg.cspace_low[1], cfg.cspace_high[1]
    x = s0 * (0.5 * (hi0 - lo0)) + 0.5 * (hi0 + lo0)
    y = s1 * (0.5 * (hi1 - lo1)) + 0.5 * (hi1 + lo1)
    ex = (x + m0 * cfg.translation_x).clamp(lo0, hi0)
    ey = (y + m1 * cfg.translation_y).clamp(lo1, hi1)
    safe = torch.ones_like(x, dtype=torch.bool)
    for b in range(pos.shape[1]):
        d = torch.hypot(pos[:, b, 0, None, None] - x, pos[:, b, 1, None, None] - y)
        safe &= (d > start_margin) | (mask[:, b, None, None] == 0)
    target = torch.arange(s, device=pos.device)[None, :] % nb[:, None]                      # [N, s]
    t = pos[torch.arange(n, device=pos.device)[:, None], target]                           # [N, s, 2]
    d1 = torch.hypot(t[..., 0, None] - x, t[..., 1, None] - y)
    d2 = torch.hypot(t[..., 0, None] - ex, t[..., 1, None] - ey)
    good = safe & ~((d1 >= motion_margin) & (d2 >= motion_margin))
    found = good.any(dim=2)
    first = torch.where(found, good.to(torch.uint8).argmax(dim=2), torch.full_like(target, attempts - 1))
    actions = torch.stack([v.gather(2, first[..., None])[..., 0] for v in (s0, s1, m0, m1)], dim=-1)
    return actions, found


def kernels(say, n, s, attempts, iters, warmup):
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0), n_envs=n, seed=5, shape_names=names)
    w = lib.World(cfg, scene, device=0)
    try:
        w.reset()
        obs = w.observe()
        pos, mask = obs['position'][..., :2].contiguous(), obs['body_mask']
        gen = torch.Generator(device=w.device); gen.manual_seed(1)
        same = lib.push_proposal_params('spread', plan_index=1, seed=1, max_attempts=attempts)
        full = lib.push_proposal_params('spread', plan_index=1, seed=1, max_attempts=20000)
        _, st_same = w.policy_heuristic_multi(same, s)
        _, st_full = w.policy_heuristic_multi(full, s)
        _, t_found = torch_proposals(pos, mask, s, attempts, cfg, 0.05, 0.01, gen)
        torch.cuda.synchronize()
        t = alternate({'k_same': lambda: w.policy_heuristic_multi(same, s), 'k_full': lambda: w.policy_heuristic_multi(full, s),
                       'torch': lambda: torch_proposals(pos, mask, s, attempts, cfg, 0.05, 0.01, gen)}, iters, warmup)
        say('--- N = %d envs, S = %d candidates, RV_HP_SPREAD, start_margin 0.05, motion_margin 0.01; %d calls each after %d warm-up'
            % (n, s, iters, warmup))
        row = '  %-58s median %9.4f ms   min %9.4f   max %9.4f'
        say(row % (('rv_policy_heuristic_multi, max_attempts %d (incl. the binding)' % attempts,) + t['k_same']))
        say(row % (('rv_policy_heuristic_multi, max_attempts 20000 (incl. the binding)',) + t['k_full']))
        say(row % (('torch: %d attempts per candidate at once, argmax' % attempts,) + t['torch']))
        say('  torch / kernel at the same budget: %.1fx;  candidates found: kernel %.2f %% (budget %d), %.2f %% (budget 20000), torch %.2f %%'
            % (t['torch'][0] / t['k_same'][0], 100.0 * float((st_same == 1).float().mean()), attempts,
               100.0 * float((st_full == 1).float().mean()), 100.0 * float(t_found.float().mean())))
        say('  attempts tried per call at budget %d: at most %.1f M (N x S x budget; a candidate stops at the round of 64 that holds its first success)'
            % (attempts, n * s * attempts / 1e6))
    finally:
        w.close()


def goal_rate(say, budget, n=64, max_steps=8):
    it, s, h = budget
    cfg = configs.push_env_config(TASK_NAME='crossing', LAYOUT_ID=0, MAX_STEPS=max_steps)
    say('--- crossing layout 0, %d envs, seed 5, one episode each of at most %d steps, gamma %.1f; %d simulated candidate steps per'
        ' decision: HeuristicShootingPushPolicy and ShootingPushPolicy S = %d, H = %d; CEMPushPolicy I = %d, S = %d, H = %d'
        ' (defaults otherwise)' % (n, max_steps, GAMMA, it * s * h, it * s, h, it, s, h))
    for name in ('heuristic', 'shooting', 'cem', 'random'):
        found = [0, 0]      # proposals found, proposals made

        def count(policy):
            found[0] += int(policy.last_found.sum()); found[1] += policy.last_found.numel()
        c = run_episodes(name, cfg, budget, GAMMA, n, max_steps, count if name == 'heuristic' else None)
        extra = '' if name != 'heuristic' else '; proposals found within max_attempts: %.2f %%' % (100.0 * found[0] / max(found[1], 1))
        say(rate_line(name, c, n, extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--attempts', type=int, default=2048)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-kernels', action='store_true')
    ap.add_argument('--skip-rate', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('push_proposals_bench: no GPU (a timing needs the device)')
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    say('tools/push_proposals_bench.py --iters %d --warmup %d --attempts %d on %s'
        % (args.iters, args.warmup, args.attempts, torch.cuda.get_device_name(0)))
    if not args.skip_kernels:
        kernels(say, 1024, 64, args.attempts, args.iters, args.warmup)
    if not args.skip_rate:
        for budget in BUDGETS:
            goal_rate(say, budget)


if __name__ == '__main__':
    main()
