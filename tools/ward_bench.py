"""Ward agglomeration of the clustered point clouds: what rv_ward_groups costs at the push config's real
clouds, and what it does where bodies touch.

    python tools/ward_bench.py [--envs 256] [--iters 10] [--warmup 2] [--steps 6] [--out profiles/ward_groups_bench.txt]

1. One chunk of --envs push envs (424 x 512 pixels each, the crop set to the table top's workspace: about 1.5 k points
   survive the plane) after a reset.  Timed alternately with device events, warm-up first, the median of --iters calls each:
   rv_segment_cloud, rv_ward_groups on its labels with k = 100 (the reference's) and with k = 10; then, on ONE env on one
   core, wall clock: the host mirror perception.point_cloud_utils.ward_labels and scikit-learn's kneighbors_graph +
   AgglomerativeClustering where it is importable, whose partition of env 0 is compared with the device's.
2. --steps steps of HeuristicPushPolicy in the same envs.  After every step the clouds are segmented both ways.  Reported:
   the share of env-steps with RV_SEG_FLAG_FEWER (fewer DBSCAN clusters than slots), the share in which one DBSCAN cluster
   holds two bodies, and on each of the two sets the purity against the renderer's segmask of the groups `largest` keeps
   and of Ward's (C = 4, and C = 5: the four bodies and the arm's link that stands inside the crop): the share of the
   clustered points that carry the majority segmask id of their group, and the number of bodies that own the majority of
   at least one group.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np
import torch

from robovat_amd import abi, configs, lib, policies
from robovat_amd.envs.push.push_env import VecPushEnv
from robovat_amd.perception import point_cloud_utils as pcu
from benchlib import alternate


def crop_config():
    from robovat_amd import scenes
    _, names = scenes.make_scene()
    ec = configs.push_env_config()
    probe = configs.make_rv_config(ec, configs.sawyer_config(), names, n_envs=1)
    c, h = list(probe.table_center), list(probe.table_half)
    ec.OBS.CROP_MIN = [c[0] - h[0], c[1] - h[1], -0.01]
    ec.OBS.CROP_MAX = [c[0] + h[0], c[1] + h[1], 0.3]
    return ec


def purity(groups, seg, n_bodies):
    """groups [m] >= 0 and segmask ids [m] of the clustered points of one env -> (points that carry their group's majority
    id, bodies that own the majority of a group)"""
    hit, owners = 0, set()
    for g in np.unique(groups):
        ids = np.bincount(seg[groups == g], minlength=256)
        hit += int(ids.max())
        if int(ids.argmax()) < n_bodies:
            owners.add(int(ids.argmax()))
    return hit, len(owners)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/ward_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/ward_bench.py --envs %d --iters %d --warmup %d --steps %d on %s'
        % (args.envs, args.iters, args.warmup, args.steps, torch.cuda.get_device_name(0)))
    n = args.envs
    env = VecPushEnv(n, config=crop_config(), seed=3)
    try:
        env.reset()
        w = env.world
        par = lib.segment_params(num_points=256)
        ward = lib.ward_params(num_points=256)
        ward10 = lib.ward_params(num_points=256, num_neighbors=10)
        ward5 = lib.ward_params(num_points=256, num_groups=abi.RV_MAXB + 1)
        depth, _ = w.render(segmask=False)
        pts, valid = w.deproject(depth)
        seg = w.segment_cloud(pts, valid, par)
        out = w.ward_groups(pts, seg['labels'], ward)
        torch.cuda.synchronize()
        info = out['info'].cpu().numpy()
        say('--- 1. N = %d envs, M = %d points each; input %.0f on average (max %d), kept %.0f, components %.2f, edges added %.2f, '
            'merges %.0f; %d envs overflow, %d with fewer points than groups, %d with a bound flag; workspace %.1f MB'
            % (n, int(pts.shape[1]), info[:, 0].mean(), int(info[:, 0].max()), info[:, 1].mean(), info[:, 2].mean(), info[:, 3].mean(),
               info[:, 4].mean(), int((info[:, 7] & abi.RV_WARD_FLAG_OVERFLOW != 0).sum()), int((info[:, 7] & abi.RV_WARD_FLAG_FEWER != 0).sum()),
               int((info[:, 7] & abi.RV_WARD_FLAG_BOUND != 0).sum()), w.lib.rv_ward_workspace_bytes(n) / 1e6))
        t = alternate({
            'segment': lambda: w.segment_cloud(pts, valid, par),
            'ward': lambda: w.ward_groups(pts, seg['labels'], ward),
            'ward10': lambda: w.ward_groups(pts, seg['labels'], ward10),
        }, args.iters, args.warmup)
        row = '  %-66s median %9.3f ms   min %9.3f   max %9.3f'
        say(row % (('rv_segment_cloud, T = 50, eps 0.02, min_samples 50, C = 4, P = 256',) + t['segment']))
        say(row % (('rv_ward_groups, k = 100, C = 4, P = 256',) + t['ward']))
        say(row % (('rv_ward_groups, k = 10',) + t['ward10']))
        say('  per env of the chunk: %.1f us (k = 100); merge steps per second and env: %.2e'
            % (1e3 * t['ward'][0] / n, info[:, 4].mean() / (t['ward'][0] * 1e-3)))
        p0 = pts[0][seg['labels'][0] >= 0].cpu().numpy()
        t0 = time.perf_counter(); pcu.ward_labels(p0, 4); t1 = time.perf_counter()
        say('  host, env 0 alone, one core: ward_labels (NumPy, %d points, k = 100) %.1f ms' % (len(p0), 1e3 * (t1 - t0)))
        try:
            import warnings
            from sklearn.cluster import AgglomerativeClustering
            from sklearn.neighbors import kneighbors_graph
            t0 = time.perf_counter()
            conn = kneighbors_graph(p0, n_neighbors=min(100, len(p0) - 1), include_self=False, n_jobs=1)
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                sk = AgglomerativeClustering(linkage='ward', n_clusters=4, connectivity=0.5 * (conn + conn.T)).fit(p0).labels_
            t1 = time.perf_counter()
            dev = out['groups'][0][seg['labels'][0] >= 0].cpu().numpy()
            agree = len(p0) <= abi.RV_WARD_MAXPTS and len(set(zip(dev.tolist(), sk.tolist()))) == len(set(dev.tolist())) == len(set(sk.tolist()))
            say("  env 0: the device's groups are scikit-learn's partition of the same %d points: %s" % (len(p0), 'yes' if agree else 'NO'))
            say('  host, env 0 alone, one core: scikit-learn kneighbors_graph + AgglomerativeClustering %.1f ms' % (1e3 * (t1 - t0)))
        except ImportError:
            say('  host: scikit-learn is not importable here; not timed')

        # ---- 2. bodies that touch
        policy = policies.HeuristicPushPolicy(env)
        n_bodies = (w.body_params()[:, :, 0] > 0).sum(dim=1).cpu().numpy()
        sets = {name: dict(steps=0, pts=0, pts_l=0, hit_l=0, hit_w=0, hit_5=0, own_l=0, own_w=0, own_5=0, bodies=0) for name in ('fewer', 'merged')}
        total = 0
        for step in range(args.steps):
            env.step(policy.action(None))
            depth, segmask = w.render()
            pts, valid = w.deproject(depth)
            r = w.segment_cloud(pts, valid, par)
            flags = r['info'][:, abi.RV_SEG_INFO_FLAGS].cpu().numpy()
            groups = w.ward_groups(pts, r['labels'], ward)['groups'].cpu().numpy()
            groups5 = w.ward_groups(pts, r['labels'], ward5)['groups'].cpu().numpy()
            labels, mask = r['labels'].cpu().numpy(), segmask.reshape(n, -1).cpu().numpy()
            slots = r['slot_labels'].cpu().numpy()
            total += n
            for e in range(n):
                keep = groups[e] >= 0      # (clustered and, where Ward thinned, kept)
                lab, grp, grp5, ids = labels[e][keep], groups[e][keep], groups5[e][keep], mask[e][keep]
                nb = int(n_bodies[e])
                merged = any(((np.bincount(ids[lab == c], minlength=256)[:nb] >= 25).sum() >= 2) for c in np.unique(lab))
                for name, on in (('fewer', bool(flags[e] & abi.RV_SEG_FLAG_FEWER)), ('merged', merged)):
                    if not on:
                        continue
                    s = sets[name]
                    in_slot = np.isin(lab, slots[e][slots[e] >= 0])      # (`largest` drops the clusters beyond its C slots)
                    hl, ol = purity(lab[in_slot], ids[in_slot], nb)
                    hw, ow = purity(grp, ids, nb)
                    h5, o5 = purity(grp5, ids, nb)
                    s['hit_5'] += h5; s['own_5'] += o5
                    s['steps'] += 1; s['pts'] += int(keep.sum()); s['pts_l'] += int(in_slot.sum()); s['hit_l'] += hl; s['hit_w'] += hw
                    s['own_l'] += ol; s['own_w'] += ow; s['bodies'] += len(set(ids[ids < nb].tolist()))
        say('--- 2. %d steps of HeuristicPushPolicy in %d envs: %d env-steps' % (args.steps, n, total))
        for name, what in (('fewer', 'with RV_SEG_FLAG_FEWER (fewer DBSCAN clusters than the %d slots)' % abi.RV_MAXB),
                           ('merged', 'in which one DBSCAN cluster holds at least 25 points of each of two bodies')):
            s = sets[name]
            say('  env-steps %s: %d (%.2f %%)' % (what, s['steps'], 100.0 * s['steps'] / total))
            if s['steps']:
                say('    purity against the segmask, largest %.4f (of the %.0f points in its slots), ward %.4f (of the %.0f clustered points); '
                    'bodies that own a group, largest %.2f, ward %.2f of %.2f bodies with clustered points (per env-step)'
                    % (s['hit_l'] / max(s['pts_l'], 1), s['pts_l'] / s['steps'], s['hit_w'] / s['pts'], s['pts'] / s['steps'],
                       s['own_l'] / s['steps'], s['own_w'] / s['steps'], s['bodies'] / s['steps']))
                say("    ward with C = %d groups (the bodies and the arm's link that stands inside the crop): purity %.4f, bodies that own "
                    "a group %.2f" % (abi.RV_MAXB + 1, s['hit_5'] / s['pts'], s['own_5'] / s['steps']))
    finally:
        env.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
