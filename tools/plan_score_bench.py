"""Time rv_plan_score against a plain-torch restatement of planning-mode PushReward on the same device.

    python tools/plan_score_bench.py [--n 1024 --s 1024 --h 8 --b 4 --task crossing --layout 0]

The torch restatement below is written from the host NumPy code (robovat_amd/reward_fns/push_reward.py) as a user
without the kernel would write it: elementwise passes over [N, S, ...] tensors, every step of every plan evaluated and
masked afterwards.  It is the yardstick, not the code under test.  The two are timed alternately with device events
(warm-up first, then the median of --iters calls each); the kernel's bytes are the plans it is given plus its three
outputs, set next to the measured HBM copy bandwidth of the MI355X (6.29 TB/s, 8.0 TB/s on paper).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robovat_amd import configs, lib, scenes  # noqa: E402
from robovat_amd.envs.push import push_layouts  # noqa: E402

HBM_MEASURED, HBM_PAPER = 6.29e12, 8.0e12
X_RANGE, Y_RANGE = (0.22, 0.98), (-0.56, 0.66)


def make_plans(torch, device, layout, n, s, h, b, high, seed=0):
    """random walks from one start per env: body 0 on a region tile, steps of up to 0.6 x the maximum stride"""
    g = torch.Generator(device=device); g.manual_seed(seed)

    def u(shape, lo, hi):
        return torch.rand(shape, generator=g, device=device) * (hi - lo) + lo
    state0 = torch.stack([u((n, b), *X_RANGE), u((n, b), *Y_RANGE)], dim=-1)
    tiles = torch.tensor(layout.offset, device=device)[None] + torch.tensor(layout.region, dtype=torch.float32, device=device) * layout.size
    state0[:, 0] = tiles[torch.randint(0, len(tiles), (n,), generator=g, device=device)] + u((n, 2), -0.4, 0.4) * layout.size
    ang = u((n, s, h, b), 0.0, 2.0 * np.pi)
    length = u((n, s, h, b), 0.0, 0.6 * (0.3 if high else 0.15)) * (torch.rand((n, s, h, b), generator=g, device=device) < 0.6)
    steps = torch.stack([length * torch.cos(ang), length * torch.sin(ang)], dim=-1)
    return state0.contiguous(), (state0[:, None, None] + torch.cumsum(steps, dim=2)).contiguous()


class TorchPlanReward(object):
    """get_reward_fn(task, layout, is_planning=True) and the return / length / arg-max recurrence in float32 torch"""

    def __init__(self, torch, device, task, layout, high, gamma):
        self.t, self.task, self.high, self.gamma = torch, task, high, gamma
        off = torch.tensor(layout.offset, device=device)

        def centres(tiles, size):
            return off[None] + torch.tensor(tiles or np.zeros((0, 2)), dtype=torch.float32, device=device).reshape(-1, 2) * size
        self.size = layout.size
        self.region, self.region125 = centres(layout.region, layout.size), centres(layout.region, layout.size * 1.25)
        self.goal = centres(layout.goal, layout.size)

    def on_tiles(self, pos, centres, max_dist):
        d = (pos[..., None, :] - centres).abs()
        return ((d[..., 0] <= 0.5 * max_dist) & (d[..., 1] <= 0.5 * max_dist)).any(dim=-1)

    def score(self, s):
        if self.task == 'clearing':
            return -self.t.minimum((s[..., 0] - 0.7).abs().mean(dim=-1), (s[..., 1] + 0.9).abs().mean(dim=-1))
        return -(s[..., 0, None, :] - self.goal).norm(dim=-1).min(dim=-1).values

    def reward(self, s, n):
        t = self.t
        lo, hi = (0.1, 0.3) if self.high else (0.01, 0.15)
        stride = (n - s).norm(dim=-1)
        term = (stride < lo).all(dim=-1) | (stride > hi).any(dim=-1)
        x, y = n[..., 0], n[..., 1]
        term = term | ((x < 0.22 - 0.02) | (x > 0.98 + 0.02) | (y < -0.56 - 0.02) | (y > 0.66 + 0.02)).any(dim=-1)
        m1, m2 = s + (1.0 / 3.0) * (n - s), s + (2.0 / 3.0) * (n - s)
        if self.task == 'insertion':
            term = term | (x[..., 0] < 0.3 - 0.02) | (x[..., 0] > 0.8 + 0.02) | (y[..., 0] < -0.56 - 0.02) | (y[..., 0] > 0.66 + 0.02)
            for p in (n, m1, m2):
                term = term | self.on_tiles(p, self.region125, self.size * 1.25).any(dim=-1)
        elif self.task == 'crossing':
            bridge = t.ones_like(term)
            for p in (n, m1, m2):
                bridge = bridge & self.on_tiles(p[..., 0, :], self.region, self.size)
            term = term | ~bridge
        if self.task == 'clearing':
            goal = ~self.on_tiles(n, self.region125, self.size * 1.25).any(dim=-1)
        else:
            goal = self.on_tiles(n[..., 0, :], self.goal, self.size)
        goal = goal & ~term
        r = 100.0 * goal.float() - 100.0 * term.float() + (self.score(n) - self.score(s)).abs() - 1.0
        return r, term | goal

    def score_plans(self, state0, plans):
        t = self.t
        N, S, H = plans.shape[:3]
        s = state0[:, None].expand(N, S, -1, -1)
        ret = t.zeros((N, S), device=plans.device); disc = 1.0
        length = t.full((N, S), H, dtype=t.int32, device=plans.device)
        alive = t.ones((N, S), dtype=t.bool, device=plans.device)
        for k in range(H):
            n = plans[:, :, k]
            r, term = self.reward(s, n)
            ret = t.where(alive, ret + disc * r, ret)
            length = t.where(alive & term, t.full_like(length, k + 1), length)
            alive = alive & ~term
            disc *= self.gamma
            s = n
        return ret, length, ret.argmax(dim=1).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1024); ap.add_argument('--s', type=int, default=1024)
    ap.add_argument('--h', type=int, default=8); ap.add_argument('--b', type=int, default=4)
    ap.add_argument('--task', default='crossing'); ap.add_argument('--layout', type=int, default=0)
    ap.add_argument('--high-level', action='store_true'); ap.add_argument('--gamma', type=float, default=0.95)
    ap.add_argument('--warmup', type=int, default=5); ap.add_argument('--iters', type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('plan_score_bench: no GPU (a timing needs the device)')
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(TASK_NAME=a.task, LAYOUT_ID=a.layout), n_envs=a.n, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    layout = push_layouts.TASK_NAME_TO_LAYOUTS[a.task][a.layout]
    state0, plans = make_plans(torch, world.device, layout, a.n, a.s, a.h, a.b, a.high_level)
    params = lib.plan_params(n_bodies=a.b, is_high_level=int(a.high_level), gamma=a.gamma)
    ref = TorchPlanReward(torch, world.device, a.task, layout, a.high_level, a.gamma)

    def run_kernel():
        return world.plan_score(plans, state0, params)

    def run_torch():
        return ref.score_plans(state0, plans)
    k_out, t_out = run_kernel(), run_torch()
    torch.cuda.synchronize()
    same_len = float((k_out[1] == t_out[1]).float().mean())
    ret_diff = float((k_out[0] - t_out[0]).abs().max())
    same_best = float((k_out[2] == t_out[2]).float().mean())
    for _ in range(a.warmup):
        run_kernel(); run_torch()
    torch.cuda.synchronize()
    times = {'kernel': [], 'torch': []}
    for _ in range(a.iters):      # alternately, so that both see the same machine
        for name, fn in (('kernel', run_kernel), ('torch', run_torch)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3)
    k_med, t_med = float(np.median(times['kernel'])), float(np.median(times['torch']))
    read = a.n * a.s * a.h * a.b * 2 * 4 + a.n * a.b * 2 * 4
    written = a.n * a.s * 8 + a.n * 4
    mean_len = float(k_out[1].float().mean())
    bw = (read + written) / k_med
    print('rv_plan_score vs a torch restatement: N=%d S=%d H=%d B=%d task=%s layout=%d high_level=%d gamma=%g' %
          (a.n, a.s, a.h, a.b, a.task, a.layout, a.high_level, a.gamma))
    print('  plans given to the kernel: %.1f MB; outputs %.1f MB; mean plan length %.2f of %d steps' % (read / 1e6, written / 1e6, mean_len, a.h))
    print('  kernel (one launch, incl. the binding):  median %.3f ms  (min %.3f, max %.3f, %d calls)' %
          (k_med * 1e3, min(times['kernel']) * 1e3, max(times['kernel']) * 1e3, a.iters))
    print('  torch restatement:                       median %.3f ms  (min %.3f, max %.3f)' %
          (t_med * 1e3, min(times['torch']) * 1e3, max(times['torch']) * 1e3))
    print('  torch / kernel: %.1fx' % (t_med / k_med))
    print('  kernel bytes/s over the plans it is given: %.2f TB/s = %.0f %% of the measured HBM copy rate (%.2f TB/s; %.1f TB/s on paper)' %
          (bw / 1e12, 100.0 * bw / HBM_MEASURED, HBM_MEASURED / 1e12, HBM_PAPER / 1e12))
    print('  (a plan that ends early is not read to its end: the rate counts bytes given, not bytes fetched)')
    print('  agreement with the restatement: lengths equal %.4f %%, best equal %.4f %%, largest return difference %.3g' %
          (100.0 * same_len, 100.0 * same_best, ret_diff))
    print(json.dumps({'n': a.n, 's': a.s, 'h': a.h, 'b': a.b, 'kernel_ms': k_med * 1e3, 'torch_ms': t_med * 1e3,
                      'bytes_given': read + written, 'kernel_tb_per_s': bw / 1e12, 'mean_length': mean_len,
                      'lengths_equal': same_len, 'best_equal': same_best, 'max_return_diff': ret_diff}))
    world.close()


if __name__ == '__main__':
    main()
