"""The depth sensor noise model on the device: what rv_depth_noise costs at the product's shape.

    python tools/depth_noise_bench.py [--envs 2048] [--height 424] [--width 512] [--iters 30] [--warmup 5]
                                      [--out profiles/depth_noise_bench.txt]

rv_depth_noise (gamma multiplier, prob 1 so that every env takes the upsampled grid, the world's own scratch grid) on
[N][H][W] float32, out of place and in place, against two baselines on the same buffers:
  * a device-to-device copy of the depth buffer (``out.copy_(depth)``): the same 4 B read + 4 B written per pixel with no
    arithmetic at all -- the floor the kernel can approach;
  * a plain-torch restatement, as a user without the kernel would write it: gamma and normal draws from torch's generator,
    multiply, ``F.interpolate(..., mode='bicubic')``, masked add.  Its cubic has a = -0.75 (Pillow's, and the kernel's,
    -0.5) and its draws are a stream, not keys: a time baseline only, it computes other numbers.
Timed alternately with device events, warm-up first, the median of --iters calls each.  Bytes/s: the bytes the algorithm
needs -- 8 B per pixel plus the grid written once and read once (8 B per grid cell) -- over the median time.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import torch

from robovat_amd import configs, lib, scenes
from benchlib import alternate


def torch_noise(depth, out, shape, prob, r, sigma, gen):
    n, h, w = depth.shape
    g = torch._standard_gamma(torch.full((n,), shape, device=depth.device), generator=gen) / shape
    applied = torch.rand((n,), generator=gen, device=depth.device) < prob
    grid = sigma * torch.randn((n, 1, h // r, w // r), generator=gen, device=depth.device)
    up = torch.nn.functional.interpolate(grid, scale_factor=r, mode='bicubic', align_corners=False)[:, 0]
    torch.mul(depth, g[:, None, None], out=out)
    return torch.where(applied[:, None, None] & (out > 0), out + up, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--height', type=int, default=424)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/depth_noise_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/depth_noise_bench.py --envs %d --height %d --width %d --iters %d --warmup %d on %s'
        % (args.envs, args.height, args.width, args.iters, args.warmup, torch.cuda.get_device_name(0)))
    n, h, w, r = args.envs, args.height, args.width, 4
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.grasp_env_config(), n_envs=n, seed=5, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    try:
        gen = torch.Generator(device=world.device); gen.manual_seed(1)
        depth = 0.4 + 0.6 * torch.rand((n, h, w), generator=gen, device=world.device)
        depth[torch.rand((n, h, w), generator=gen, device=world.device) < 0.1] = 0.0
        out = torch.empty_like(depth)
        work = depth.clone()
        p = lib.depth_noise_params({'GAMMA_SHAPE': 1000.0, 'PROB': 1.0, 'RESCALE_FACTOR': r, 'SIGMA': 0.005, 'SEED': 1})
        off = lib.depth_noise_params({'GAMMA_SHAPE': 1000.0, 'PROB': 0.0, 'RESCALE_FACTOR': r, 'SIGMA': 0.005, 'SEED': 1})
        # the kernel and the torch baseline agree on what they do to the image: the same pixels change, by the same spread
        k_out, g, applied, grid = world.depth_noise(depth, p, record=True)
        t_out = torch_noise(depth, out, 1000.0, 1.0, r, 0.005, gen)
        torch.cuda.synchronize()
        kd, td = (k_out - depth)[depth > 0], (t_out - depth)[depth > 0]
        say('--- agreement in kind: kernel noise on hit pixels mean %.2e std %.4f; torch baseline mean %.2e std %.4f; zero pixels '
            'changed: %d / %d' % (float(kd.mean()), float(kd.std()), float(td.mean()), float(td.std()),
                                  int((k_out[depth == 0] != 0).sum()), int((t_out[depth == 0] != 0).sum())))
        del k_out, t_out, kd, td, grid
        t = alternate({
            'kernel': lambda: world.depth_noise(depth, p, out=out),
            'inplace': lambda: world.depth_noise(work, p, out=work),
            'gamma_only': lambda: world.depth_noise(depth, off, out=out),
            'copy': lambda: out.copy_(depth),
            'torch': lambda: torch_noise(depth, out, 1000.0, 1.0, r, 0.005, gen),
        }, args.iters, args.warmup)
        px = n * h * w
        need = 8.0 * px + 8.0 * px / (r * r)
        say('--- N = %d, %d x %d, R = %d (grid %d x %d): %.1f MB per buffer; %d calls each after %d warm-up'
            % (n, h, w, r, h // r, w // r, 4.0 * px / 1e6, args.iters, args.warmup))
        row = '  %-58s median %8.3f ms   min %8.3f   max %8.3f   %6.2f TB/s'
        say(row % (('rv_depth_noise, prob 1 (two launches, incl. the binding)',) + t['kernel'] + (need / t['kernel'][0] / 1e9,)))
        say(row % (('rv_depth_noise, prob 1, in place',) + t['inplace'] + (need / t['inplace'][0] / 1e9,)))
        say(row % (('rv_depth_noise, prob 0 (the gamma product alone)',) + t['gamma_only'] + (8.0 * px / t['gamma_only'][0] / 1e9,)))
        say(row % (('device-to-device copy of the depth buffer',) + t['copy'] + (8.0 * px / t['copy'][0] / 1e9,)))
        say(row % (('torch: draws, multiply, interpolate(bicubic), masked add',) + t['torch'] + (need / t['torch'][0] / 1e9,)))
        say('  copy / kernel %.2f (1 = the floor), torch / kernel %.1fx; bytes needed per call %.1f MB (8 B per pixel + 8 B per grid cell)'
            % (t['copy'][0] / t['kernel'][0], t['torch'][0] / t['kernel'][0], need / 1e6))
    finally:
        world.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
