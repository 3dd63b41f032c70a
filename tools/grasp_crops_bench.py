"""Grasp-centred depth crops on the device: what rv_grasp_crops costs at the product's shape, and what a
labelled grasp set costs to collect.

    python tools/grasp_crops_bench.py [--envs 2048] [--k 16] [--iters 20] [--warmup 3] [--samples 3] [--skip-samples]
                                      [--out profiles/grasp_crops_bench.txt]

N config-4 grasp envs are reset and rendered once (424 x 512), rv_policy_antipodal_multi gives K image grasps per env, and
rv_grasp_crops is timed at two shapes -- 32 x 32 step 3 (the binding's default) and 96 x 96 step 1 (the same window at
full resolution) -- against two yardsticks in the same process:
  * a plain-torch restatement, as a user without the kernel would write it on the device: the index arithmetic in float32
    tensors of [N, K, h, w] plus advanced indexing.  It computes the same numbers (the tool counts the pixels that differ);
  * a device-to-device copy of a buffer of the output's size (``other.copy_(images)``): as many bytes written as the kernel
    writes and as many read, with no arithmetic and no gather -- the byte floor.
Timed alternately with device events, warm-up first, the median with min and max of --iters calls each.  GB/s: the output's
bytes over the median time (the kernel also reads: a gather from a window of the depth image that the caches serve).
Then ``VecGrasp4DofEnv.collect_grasp_samples(K)`` -- render, sampler, crops, N x K trial grasps -- in wall-clock seconds per
call (the median of --samples calls after one warm-up call that also builds the N x K world), as samples per second, with
the share of valid samples whose trial grasp earned a positive reward.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from robovat_amd import lib
from robovat_amd.envs.grasp.grasp_4dof_env import VecGrasp4DofEnv
from benchlib import alternate

SHAPES = [(32, 32, 3), (96, 96, 1)]


def torch_crops(depth, grasps, h, w, step):
    """rv_grasp_crops in plain torch: the arithmetic of csrc/rv_dev_grasp_sampler.h on float32 tensors, then one gather"""
    n, H, W = depth.shape
    x1, y1, x2, y2 = (grasps[:, :, i, None, None] for i in range(4))
    ax, ay = x2 - x1, y2 - y1
    ln = torch.sqrt(ax * ax + ay * ay)
    ok = (ln > 0) & torch.isfinite(ln)
    safe = torch.where(ok, ln, torch.ones_like(ln))
    c = torch.where(ok, ax / safe, torch.ones_like(ln))
    s = torch.where(ok, ay / safe, torch.zeros_like(ln))
    gx, gy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    x0 = float(np.floor(0.5 * W - 0.5 * w * step) - 0.5 * W)
    y0 = float(np.floor(0.5 * H - 0.5 * h * step) - 0.5 * H)
    ox = (x0 + torch.arange(w, device=depth.device, dtype=torch.float32) * step + step // 2).reshape(1, 1, 1, w)
    oy = (y0 + torch.arange(h, device=depth.device, dtype=torch.float32) * step + step // 2).reshape(1, 1, h, 1)
    sx = (c * ox - s * oy) + gx
    sy = (s * ox + c * oy) + gy
    inside = (sx >= -0.5) & (sx < W - 0.5) & (sy >= -0.5) & (sy < H - 0.5)
    ix = torch.where(inside, torch.floor(sx + 0.5), torch.zeros_like(sx)).long().clamp_(0, W - 1)
    iy = torch.where(inside, torch.floor(sy + 0.5), torch.zeros_like(sy)).long().clamp_(0, H - 1)
    env = torch.arange(n, device=depth.device).reshape(n, 1, 1, 1)
    return torch.where(inside, depth[env, iy, ix], torch.zeros((), device=depth.device))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--samples', type=int, default=3)
    ap.add_argument('--skip-samples', action='store_true', help='the kernel timings only (a profiler run)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/grasp_crops_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/grasp_crops_bench.py --envs %d --k %d --iters %d --warmup %d --samples %d%s on %s'
        % (args.envs, args.k, args.iters, args.warmup, args.samples, ' --skip-samples' if args.skip_samples else '',
           torch.cuda.get_device_name(0)))
    n, k = args.envs, args.k
    env = VecGrasp4DofEnv(n, seed=5)
    try:
        env.reset()
        world = env.world
        depth, _ = world.render()
        env.sample_antipodal_candidates(k, depth=depth)
        grasps = env.antipodal_image_grasps
        found = int((env.antipodal_status == 1).sum())
        say('--- N = %d config-4 grasp envs, depth %d x %d (%.1f MB), K = %d image grasps per env (%d envs found a grasp, mean count %.1f)'
            % (n, depth.shape[1], depth.shape[2], 4.0 * depth.numel() / 1e6, k, found, float(env.antipodal_count.float().mean())))
        for h, w, step in SHAPES:
            p = lib.grasp_crop_params(h, w, step)
            out, _ = world.grasp_crops(depth, grasps, p)
            ref = torch_crops(depth, grasps, h, w, step)
            torch.cuda.synchronize()
            differ = int((out != ref).sum())
            other = torch.empty_like(out)
            del ref
            t = alternate({
                'kernel': lambda: world.grasp_crops(depth, grasps, p, out=out, grasp_depths=False),
                'copy': lambda: other.copy_(out),
                'torch': lambda: torch_crops(depth, grasps, h, w, step),
            }, args.iters, args.warmup)
            nbytes = 4.0 * out.numel()
            say('--- %d x %d step %d: %d images, output %.1f MB; %d pixels of %d differ from the torch restatement; %d calls each '
                'after %d warm-up' % (h, w, step, n * k, nbytes / 1e6, differ, out.numel(), args.iters, args.warmup))
            row = '  %-62s median %8.3f ms   min %8.3f   max %8.3f   %8.1f GB/s of output'
            say(row % (('rv_grasp_crops (one launch, incl. the binding)',) + t['kernel'] + (nbytes / t['kernel'][0] / 1e6,)))
            say(row % (('device-to-device copy of a buffer of the output\'s size',) + t['copy'] + (nbytes / t['copy'][0] / 1e6,)))
            say(row % (('torch: index arithmetic + advanced indexing',) + t['torch'] + (nbytes / t['torch'][0] / 1e6,)))
            say('  kernel / copy %.2f (1 = the byte floor), torch / kernel %.1fx' % (t['kernel'][0] / t['copy'][0], t['torch'][0] / t['kernel'][0]))
            del out, other
        if args.skip_samples:
            say('--- collect_grasp_samples: unmeasured (--skip-samples)')
        else:
            s = env.collect_grasp_samples(k)      # (warm-up: builds the N x K world)
            torch.cuda.synchronize()
            wall = []
            for _ in range(args.samples):
                t0 = time.perf_counter()
                s = env.collect_grasp_samples(k)
                torch.cuda.synchronize()
                wall.append(time.perf_counter() - t0)
            med = float(np.median(wall))
            valid = s['valid']
            nv = int(valid.sum())
            pos = int((s['rewards'][valid] > 0).sum())
            say('--- collect_grasp_samples(%d), 32 x 32 step 3: %.3f s per call (min %.3f, max %.3f, %d calls after 1 warm-up): '
                '%.0f samples/s of %d, %.0f valid samples/s' % (k, med, min(wall), max(wall), args.samples, n * k / med, n * k, nv / med))
            say('  valid samples %d of %d (%.1f %%); of the valid ones %d earned a positive reward (%.1f %%)'
                % (nv, n * k, 100.0 * nv / (n * k), pos, 100.0 * pos / max(nv, 1)))
    finally:
        env.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
