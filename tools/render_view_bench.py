"""Free camera views on the device: what rv_render_view costs next to rv_render_rgb, what supersampling
costs, and what recording a step costs.

    python tools/render_view_bench.py [--iters 20] [--warmup 3] [--record-envs 1024] [--reps 3] [--skip-record]
                                      [--out profiles/render_view_bench.txt]

(a) 64 push envs at their own cameras at the config's 424 x 512: ``rv_render_view`` against ``rv_render_rgb`` in the same
    process, timed alternately with device events (warm-up first; median, min and max of --iters calls each).  The two do
    the same work per pixel and must give the same picture (the tool compares).  Both calls include k_obs_snap.
(b) 16 views (four cameras on each of four envs) at 480 x 640 with supersample 1, 2 and 4, as rays per second: views x
    pixels x s x s over the median time.
(c) wall-clock seconds of ``VecPushEnv.record_step`` at --record-envs envs with 4 recorded envs and every = 25 (64 x 48
    frames, at most 256 of them) against the plain ``step()`` of the same actions on a twin: what watching four envs adds to
    a step of the batch -- copying their blocks, stepping the copies in polls of 25 substeps, a render per poll.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from robovat_amd import lib
from robovat_amd.envs.push.push_env import VecPushEnv
from robovat_amd.perception import camera_row, look_at
from benchlib import alternate, wall


def views(cfg, height, width):
    """four cameras around the table of ``cfg``, all looking at the point 5 cm above its centre"""
    c = np.array([cfg.table_center[0], cfg.table_center[1], float(cfg.table_z)])
    eyes = [((0.9, -0.9, 0.7), (0, 0, 1)), ((-0.2, 1.1, 0.5), (0, 0, 1)), ((0.0, 0.0, 1.3), (1, 0, 0)), ((1.2, 0.1, 0.25), (0, 0, 1))]
    return np.stack([camera_row(look_at(c + np.array(e), c + np.array([0, 0, 0.05]), up=up, height=height, width=width, fov_y_deg=45.0))
                     for e, up in eyes])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--record-envs', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--skip-record', action='store_true', help='the kernel timings only (a profiler run)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/render_view_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/render_view_bench.py --iters %d --warmup %d --record-envs %d --reps %d%s on %s'
        % (args.iters, args.warmup, args.record_envs, args.reps, ' --skip-record' if args.skip_record else '', torch.cuda.get_device_name(0)))
    row = '  %-58s median %8.3f ms   min %8.3f   max %8.3f'
    env = VecPushEnv(64, seed=5)
    try:
        env.reset()
        world = env.world
        cfg = env.rv_config
        H, W = int(cfg.cam_height), int(cfg.cam_width)
        own = np.ascontiguousarray(world.camera().cpu().numpy(), dtype=np.float32)
        ours = world.render_view(own)['rgb']
        theirs = world.render_rgb()
        torch.cuda.synchronize()
        say('--- (a) 64 push envs at their own cameras, %d x %d, rgb: %d of %d bytes differ; %d calls each after %d warm-up'
            % (H, W, int((ours != theirs).sum()), ours.numel(), args.iters, args.warmup))
        idx = np.arange(64, dtype=np.int32)

        p = lib.view_params(64, H, W)

        def view():
            world.lib.rv_render_view(world.h, C.byref(p), idx.ctypes.data_as(C.c_void_p), own.ctypes.data_as(C.c_void_p),
                                     world._ptr(ours), None, None)

        def rgb():
            world.lib.rv_render_rgb(world.h, world._ptr(theirs))
        t = alternate({'view': view, 'rgb': rgb}, args.iters, args.warmup)
        rays = 64.0 * H * W
        say(row % (('rv_render_view (one launch + k_obs_snap)',) + t['view']) + '   %7.2f Grays/s' % (rays / t['view'][0] / 1e6))
        say(row % (('rv_render_rgb (one launch + k_obs_snap)',) + t['rgb']) + '   %7.2f Grays/s' % (rays / t['rgb'][0] / 1e6))
        say('  view / rgb %.3f (medians); the spread of either is its min and max above' % (t['view'][0] / t['rgb'][0]))
        h2, w2 = 480, 640
        rows = np.tile(views(cfg, h2, w2), (4, 1))
        idx16 = np.repeat(np.arange(4, dtype=np.int32), 4)
        out = torch.empty((16, h2, w2, 3), dtype=torch.uint8, device=world.device)
        say('--- (b) 16 views (4 cameras x 4 envs) at %d x %d, rgb' % (h2, w2))
        fns = dict(('s = %d' % s, (lambda s=s: world.render_view(rows, idx16, h2, w2, supersample=s, out={'rgb': out}))) for s in (1, 2, 4))
        t = alternate(fns, args.iters, args.warmup)
        for s in (1, 2, 4):
            k = 's = %d' % s
            say(row % (('supersample %d (%d rays per pixel)' % (s, s * s),) + t[k]) + '   %7.2f Grays/s' % (16.0 * h2 * w2 * s * s / t[k][0] / 1e6))
    finally:
        env.close()
    if args.skip_record:
        say('--- (c) record_step: unmeasured (--skip-record)')
    else:
        n = args.record_envs
        env, twin = VecPushEnv(n, seed=5), VecPushEnv(n, seed=5)
        try:
            env.reset(); twin.reset()
            cams = views(env.rv_config, 48, 64)[:1]
            watched = [0, n // 3, (2 * n) // 3, n - 1]
            frames = []

            def rec():
                o = env.record_step(env.sample_random_actions(), cams, watched, 25, 48, 64)
                frames.append(o[3]['num_frames'])

            def plain():
                twin.step(twin.sample_random_actions())
            t_rec, t_plain = wall(rec, args.reps), wall(plain, args.reps)
            same = bool((env.world.save_state().blocks == twin.world.save_state().blocks).all())
            say('--- (c) %d push envs, 4 recorded (rows %s), every = 25, 48 x 64 frames: %d calls each after 1 warm-up (successive steps of one '
                'episode)' % (n, watched, args.reps))
            say('  record_step %.3f s per call, plain step() %.3f s per call: + %.3f s (x %.2f); frames per call %s; env blocks equal the '
                'twin\'s afterwards: %s' % (t_rec, t_plain, t_rec - t_plain, t_rec / t_plain, frames, same))
        finally:
            env.close(); twin.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
