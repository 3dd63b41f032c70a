"""Point clouds segmented without the segmask: what rv_deproject and rv_segment_cloud cost at the push config's
real clouds.

    python tools/segment_bench.py [--envs 256] [--iters 10] [--warmup 2] [--out profiles/segment_cloud_bench.txt]

One chunk of --envs push envs (424 x 512 pixels each) after a reset, twice: with the crop set to the table top's workspace
(what a user of the real sensor sets: about 1.5 k points survive the plane) and without a crop (table sides, arm and all:
the survivors overflow RV_SEG_MAXPTS in most envs, the worst case of the pair loops).  Timed alternately with device events,
warm-up first, the median of --iters calls each:
  * rv_render, rv_deproject, rv_segment_cloud, and rv_segment_cloud with T = 0 (no plane stage) and with min_samples so
    large that nothing is core (the count pass alone of the three pair passes);
  * a plain-torch restatement of stage 1 (the 50 hypotheses scored on the same [N][M] cloud, a loop over hypotheses) and of
    the neighbour count (cdist on the kept points, env by env) -- what a user without the kernel would write; it stops short
    of the components, the borders and the sampling;
  * the host pipeline on ONE env on one core: perception.point_cloud_utils.remove_table, then scikit-learn's DBSCAN where
    it is importable (wall clock).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from robovat_amd import abi, configs, lib, scenes
from robovat_amd.perception import point_cloud_utils as pcu
from benchlib import alternate


def make_world(n, crop):
    scene, names = scenes.make_scene()
    ec = configs.push_env_config()
    if crop:
        probe = configs.make_rv_config(ec, configs.sawyer_config(), names, n_envs=1)
        c, h = list(probe.table_center), list(probe.table_half)
        ec.OBS.CROP_MIN = [c[0] - h[0], c[1] - h[1], -0.01]
        ec.OBS.CROP_MAX = [c[0] + h[0], c[1] + h[1], 0.3]
    cfg = configs.make_rv_config(ec, configs.sawyer_config(), names, n_envs=n, seed=3)
    w = lib.World(cfg, scene, device=0)
    w.reset()
    return w


def torch_plane(pts, valid, a, nv, thresh):
    """scores [N, T] of the hypotheses (a, nv [N, T, 3]) on pts [N, M, 3]"""
    scores = []
    for h in range(a.shape[1]):
        d = ((pts - a[:, h, None, :]) * nv[:, h, None, :]).sum(-1)
        scores.append(((d * d <= thresh * thresh * (nv[:, h] * nv[:, h]).sum(-1)[:, None]) & valid).sum(-1))
    return torch.stack(scores, dim=1)


def torch_counts(kept, eps):
    """neighbour counts of every env's kept points (a list of [K, 3])"""
    return [(torch.cdist(k, k) <= eps).sum(-1) for k in kept]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/segment_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/segment_bench.py --envs %d --iters %d --warmup %d on %s' % (args.envs, args.iters, args.warmup, torch.cuda.get_device_name(0)))
    n = args.envs
    for crop in (True, False):
        w = make_world(n, crop)
        try:
            depth, _ = w.render(segmask=False)
            pts, valid = w.deproject(depth)
            m = int(pts.shape[1])
            par = lib.segment_params(num_points=256)
            no_plane = lib.segment_params(num_points=256, num_hypotheses=0)
            count_only = lib.segment_params(num_points=256, min_samples=1 << 30)
            out = w.segment_cloud(pts, valid, par)
            torch.cuda.synchronize()
            info = out['info'].cpu().numpy()
            labels = out['labels']
            kept = info[:, abi.RV_SEG_INFO_KEPT].astype(np.float64)
            say('--- %s: N = %d envs, M = %d points each; valid %.0f, on the plane %.0f, survivors %.0f, kept %.0f (max %d), clusters %.1f, '
                'noise %.0f on average; %d envs overflow, %d with fewer clusters than slots, %d with a bound flag'
                % ('crop = the table top workspace' if crop else 'no crop', n, m, info[:, 0].mean(), info[:, 1].mean(), info[:, 2].mean(),
                   kept.mean(), int(kept.max()), info[:, 4].mean(), info[:, 5].mean(),
                   int((info[:, 7] & abi.RV_SEG_FLAG_OVERFLOW != 0).sum()), int((info[:, 7] & abi.RV_SEG_FLAG_FEWER != 0).sum()),
                   int((info[:, 7] & abi.RV_SEG_FLAG_BOUND != 0).sum())))
            # the torch restatement's inputs: three random points of the env stand in for a hypothesis' keyed triple
            t_hyp = 50
            gen = torch.Generator(device=w.device); gen.manual_seed(1)
            pick = torch.randint(0, m, (n, t_hyp, 3), generator=gen, device=w.device)
            tri = pts[torch.arange(n, device=w.device)[:, None, None], pick]      # [N, T, 3, 3]
            a_h = tri[:, :, 0].contiguous()
            nv_h = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1).contiguous()
            vmask = valid != 0
            kept_pts = [pts[e][labels[e] >= -1] for e in range(n)]
            t = alternate({
                'render': lambda: w.render(segmask=False),
                'deproject': lambda: w.deproject(depth),
                'segment': lambda: w.segment_cloud(pts, valid, par),
                'no_plane': lambda: w.segment_cloud(pts, valid, no_plane),
                'count_only': lambda: w.segment_cloud(pts, valid, count_only),
                'torch_plane': lambda: torch_plane(pts, vmask, a_h, nv_h, 0.015),
                'torch_counts': lambda: torch_counts(kept_pts, 0.02),
            }, args.iters, args.warmup)
            row = '  %-66s median %9.3f ms   min %9.3f   max %9.3f'
            say(row % (('rv_render (depth only)',) + t['render']))
            say(row % (('rv_deproject',) + t['deproject']))
            say(row % (('rv_segment_cloud, T = 50, eps 0.02, min_samples 50, C = 4, P = 256',) + t['segment']))
            say(row % (('rv_segment_cloud, T = 0 (no plane stage; everything survives)',) + t['no_plane']))
            say(row % (('rv_segment_cloud, nothing core (plane + the count pass alone)',) + t['count_only']))
            say(row % (('torch: 50 hypotheses scored on the same cloud (stage 1 alone)',) + t['torch_plane']))
            say(row % (('torch: neighbour counts by cdist on the kept points, env by env',) + t['torch_counts']))
            pairs = float((kept * kept).sum())
            say('  kept pairs (sum of kept^2) %.3e: the count pass alone runs at %.2e pair tests/s if it were all of its call; '
                'bytes the call must read: %.1f MB (points + mask, read by the valid scan, the scoring and the survivor pass)'
                % (pairs, pairs / (t['count_only'][0] * 1e-3), n * m * 13.0 / 1e6))
            say('  torch stage 1 + counts / kernel: %.1fx' % ((t['torch_plane'][0] + t['torch_counts'][0]) / t['segment'][0]))
            if crop:
                # the host pipeline on env 0, one core
                p0 = pts[0][valid[0] != 0].cpu().numpy()
                t0 = time.perf_counter(); rest = pcu.remove_table(p0, seed=3); t1 = time.perf_counter()
                say('  host, env 0 alone, one core: remove_table (NumPy, 50 hypotheses, %d points) %.1f ms' % (len(p0), 1e3 * (t1 - t0)))
                try:
                    from sklearn.cluster import DBSCAN
                    t0 = time.perf_counter(); DBSCAN(eps=0.02, min_samples=50, n_jobs=1).fit(rest); t1 = time.perf_counter()
                    say('  host, env 0 alone, one core: scikit-learn DBSCAN on the %d survivors %.1f ms' % (len(rest), 1e3 * (t1 - t0)))
                except ImportError:
                    say('  host: scikit-learn is not importable here; DBSCAN not timed')
        finally:
            w.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
