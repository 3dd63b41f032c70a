"""Cross-entropy refinement of grasp candidates on the device: what the step between two scorings costs,
and what the refinement is worth.

    python tools/grasp_refine_bench.py [--envs 2048] [--iters 20] [--warmup 3] [--skip-policy] [--collect 3] [--epochs 6]
                                       [--eval-envs 1024] [--out profiles/grasp_refine_bench.txt]

(a) N config-4 grasp envs are reset and rendered once; rv_policy_antipodal_multi gives K image grasps per env, K = 16 and
    K = 64.  rv_grasp_refine (one launch: rank, elites, children with the sampler's checks, world actions) is timed against
    a torch restatement of the same step on the same device (sort, gathers, normals from torch.randn, the 4 x 4 depth
    window by sixteen gathers, the 4-DoF conversion: eager kernels) and next to one iteration's scoring, rv_grasp_crops +
    rv_grasp_quality with the default model -- called in turn, device events, warm-up first, median with min and max of
    --iters calls each.
(b) the success table of tools/grasp_quality_bench.py (the same collected set, training recipe, 1024 scenes of seed 1005,
    one reset and one step each) with rows for CEMGraspPolicy: score='model' at 1, 2 and 3 iterations, score='simulator' at
    2 iterations; wall clock of one ``policy.action`` each.  No threshold is set for either number.
"""
import argparse
import importlib.util
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import numpy as np
import torch

from robovat_amd import configs, lib, policies
from robovat_amd.envs.grasp.grasp_4dof_env import VecGrasp4DofEnv
from robovat_amd.perception.grasp_quality import GraspQualityModel
from benchlib import alternate, wall

SIGMAS = (3.0, 0.15, 0.005)


def torch_step(depth, grasps, scores, count, status, cam, n_elites, sigmas, sampler):
    """the step of rv_grasp_refine in eager torch (normals from torch.randn: the same work, not the same draws)"""
    n, k, _ = grasps.shape
    H, W = depth.shape[1:]
    r0, c0, r1, c1 = sampler['CROP'] if sampler.get('CROP') is not None else (0, 0, H, W)
    j = torch.arange(k, device=depth.device)
    cand = (status == 1)[:, None] & (j[None, :] < count[:, None])
    v = cand.sum(dim=1)
    key = torch.where(cand, torch.nan_to_num(scores, nan=-3.0e38), torch.full_like(scores, -3.4e38))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    ep = torch.clamp(v, min=1, max=n_elites)
    r = torch.where(j[None, :] < ep[:, None], j[None, :].expand(n, k), (j[None, :] - ep[:, None]) % ep[:, None])
    e = order.gather(1, r)
    p = grasps.gather(1, e[:, :, None].expand(n, k, 5))
    z = torch.randn((n, k, 4), device=depth.device, dtype=torch.float32)
    g = 0.5 * (p[..., 0:2] + p[..., 2:4])
    a = 0.5 * (p[..., 2:4] - p[..., 0:2])
    c = g + sigmas[0] * z[..., 0:2]
    dl = sigmas[1] * z[..., 2]
    cs, sn = torch.cos(dl), torch.sin(dl)
    b = torch.stack([cs * a[..., 0] - sn * a[..., 1], sn * a[..., 0] + cs * a[..., 1]], dim=-1)
    p1, p2 = c - b, c + b
    u = 0.5 * (p1 + p2)
    ux, uy = u[..., 0], u[..., 1]
    inside = (ux >= c0) & (ux <= c1) & (uy >= r0) & (uy <= r1)
    dist = torch.minimum(torch.minimum((uy - r0).abs(), (ux - c0).abs()), torch.minimum((uy - r1).abs(), (ux - c1).abs()))
    wh, ww = int(sampler['DEPTH_SAMPLE_WINDOW_HEIGHT']), int(sampler['DEPTH_SAMPLE_WINDOW_WIDTH'])
    ok = inside & (dist >= float(sampler['MIN_DIST_FROM_BOUNDARY']))
    y0 = torch.where(ok, uy - wh, torch.zeros_like(uy)).long().clamp(0, H - 2 * wh)
    x0 = torch.where(ok, ux - ww, torch.zeros_like(ux)).long().clamp(0, W - 2 * ww)
    flat = depth.reshape(n, H * W)
    cd = torch.full_like(ux, float('inf'))
    for dy in range(2 * wh):
        for dx in range(2 * ww):
            cd = torch.minimum(cd, flat.gather(1, (y0 + dy) * W + x0 + dx))
    ok = ok & (cd != 0) & ~torch.isnan(cd)
    zc = torch.minimum(torch.maximum(p[..., 4] + sigmas[2] * z[..., 3], cd + float(sampler['MIN_DEPTH_OFFSET'])),
                       cd + float(sampler['MAX_DEPTH_OFFSET']))
    child = torch.cat([p1, p2, zc[..., None]], dim=-1)
    ok = ok & torch.isfinite(child).all(dim=-1)
    is_child = (j[None, :] >= ep[:, None]) & (v > 0)[:, None]
    keep = is_child & ok
    rows = torch.where(keep[..., None], child, p)
    rows = torch.where((v > 0)[:, None, None], rows, grasps)
    parent = torch.where(is_child & ~ok, -1 - e, e)
    parent = torch.where((v > 0)[:, None], parent, j[None, :].expand(n, k)).to(torch.int32)
    # ap_grasp_4dof
    fx, fy, cx, cy, sk = [cam[:, i, None] for i in range(5)]
    R, t = cam[:, 5:14], cam[:, 14:17]
    uu, vv, zz = 0.5 * (rows[..., 0] + rows[..., 2]), 0.5 * (rows[..., 1] + rows[..., 3]), rows[..., 4]
    yc = (vv - cy) / fy
    xc = (uu - cx - sk * yc) / fx
    q = torch.stack([zz * xc - t[:, 0, None], zz * yc - t[:, 1, None], zz - t[:, 2, None]], dim=-1)
    xyz = torch.einsum('nkr,nrc->nkc', q, R.reshape(n, 3, 3))
    phi = torch.atan2(rows[..., 3] - rows[..., 1], rows[..., 2] - rows[..., 0]) + 0.5 * np.pi
    m00 = R[:, 0, None] * torch.cos(phi) + R[:, 3, None] * torch.sin(phi)
    m10 = R[:, 1, None] * torch.cos(phi) + R[:, 4, None] * torch.sin(phi)
    yaw = torch.atan2(m10, m00)
    count_out = torch.where(v > 0, torch.full_like(count, k), torch.zeros_like(count))
    return rows, torch.cat([xyz, yaw[..., None]], dim=-1), parent, count_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--collect', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--skip-policy', action='store_true', help='the kernel half only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/grasp_refine_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    say('tools/grasp_refine_bench.py --envs %d --iters %d --warmup %d --collect %d --epochs %d --eval-envs %d%s on %s'
        % (args.envs, args.iters, args.warmup, args.collect, args.epochs, args.eval_envs,
           ' --skip-policy' if args.skip_policy else '', torch.cuda.get_device_name(0)))
    n = args.envs
    sampler = configs.ANTIPODAL_GRASP_4DOF_POLICY_CONFIG['SAMPLER']
    sp = lib.antipodal_params()
    model = GraspQualityModel.random_init(1, norm=dict(im_mean=0.6, im_inv_std=8.0, z_mean=0.6, z_inv_std=20.0))
    env = VecGrasp4DofEnv(n, seed=5)
    sets = []
    try:
        env.reset()
        world = env.world
        depth, _ = world.render()
        cam = world.camera()
        # ---- (a) the kernel
        for k in (16, 64):
            e = max(1, k // 4)
            env.sample_antipodal_candidates(k, depth=depth)
            g, cnt, st = env.antipodal_image_grasps, env.antipodal_count, env.antipodal_status
            scores = torch.randn((n, k), generator=torch.Generator(device=world.device).manual_seed(k), device=world.device)
            params = lib.grasp_refine_params(n_elites=e, sigma_center=SIGMAS[0], sigma_angle=SIGMAS[1], sigma_depth=SIGMAS[2], iteration=1)
            out = world.grasp_refine(depth, g, scores, params, sp, count=cnt, status=st, actions4=True)
            ref = torch_step(depth, g, scores, cnt, st, cam, e, SIGMAS, sampler)
            torch.cuda.synchronize()
            par, rpar = out[2].cpu().numpy(), ref[2].cpu().numpy()
            elite_same = bool(np.array_equal(par[:, :1], rpar[:, :1]))
            say('--- (a) %d envs x K = %d, E = %d: %d candidates, %d of %d children accepted by the kernel (torch, other draws: %d); '
                'best elite the same in both: %s' % (n, k, e, int(cnt.sum()), int((par[:, e:] >= 0).sum()), n * (k - e),
                                                    int((rpar[:, e:] >= 0).sum()), elite_same))
            fns = {'kernel': lambda: world.grasp_refine(depth, g, scores, params, sp, count=cnt, status=st, actions4=True),
                   'torch': lambda: torch_step(depth, g, scores, cnt, st, cam, e, SIGMAS, sampler),
                   'scoring': lambda: env.grasp_qualities(model, g, depth)}
            t = alternate(fns, args.iters, args.warmup)
            row = '  %-66s median %8.3f ms   min %8.3f   max %8.3f'
            say(row % (('rv_grasp_refine (one launch, incl. the binding and 4 allocations)',) + t['kernel']))
            say(row % (('torch restatement of the step (eager)',) + t['torch']))
            say(row % (('one scoring: rv_grasp_crops + rv_grasp_quality, default model',) + t['scoring']))
            say('  torch / kernel %.1fx;  kernel / scoring %.3f (the share the new step adds to an iteration)'
                % (t['torch'][0] / t['kernel'][0], t['kernel'][0] / t['scoring'][0]))
        flush()
        if args.skip_policy:
            say('--- (b) refinement: unmeasured (--skip-policy)')
        else:
            k = 16
            t0 = time.perf_counter()
            for i in range(args.collect):
                if i:
                    env.reset()
                s = env.collect_grasp_samples(k)
                v = s['valid'].cpu().numpy()
                sets.append((s['images'].cpu().numpy()[v], s['grasp_depths'].cpu().numpy()[v], (s['rewards'].cpu().numpy()[v] > 0).astype(np.float32)))
            say('--- (b) collected %d valid samples in %d calls of collect_grasp_samples(%d) on %d envs, %.1f s'
                % (sum(len(a[2]) for a in sets), args.collect, k, n, time.perf_counter() - t0))
    finally:
        env.close()
    if args.skip_policy:
        flush()
        return
    x, z, y = (np.concatenate([a[i] for a in sets]) for i in range(3))
    say('  positive share of the labels %.1f %%' % (100.0 * y.mean()))
    spec = importlib.util.spec_from_file_location('train_grasp_quality', os.path.join(HERE, 'train_grasp_quality.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t0 = time.perf_counter()
    trained, history = tool.train(x, z, y, epochs=args.epochs, batch=256, lr=1e-3, seed=0, log=lambda s: say('  ' + s))
    say('  trained %d epochs on the CPU in %.1f s' % (args.epochs, time.perf_counter() - t0))
    ne, k = args.eval_envs, 16
    makers = [('candidate 0 (AntipodalGrasp4DofPolicy)', lambda e: policies.AntipodalGrasp4DofPolicy(e)),
              ('GraspQualityPolicy, K = %d, trained model' % k, lambda e: policies.GraspQualityPolicy(e, trained, k)),
              ('GraspQualityPolicy, K = %d, untrained model (seed 1)' % k, lambda e: policies.GraspQualityPolicy(e, model, k)),
              ('LookaheadGrasp4DofPolicy, K = %d (executes all K)' % k, lambda e: policies.LookaheadGrasp4DofPolicy(e, k))]
    for its in (0, 1, 2, 3):
        makers.append(('CEMGraspPolicy model, K = %d, %d iteration%s, trained model' % (k, its, '' if its == 1 else 's'),
                       lambda e, its=its: policies.CEMGraspPolicy(e, k, num_iterations=its, model=trained)))
    makers.append(('CEMGraspPolicy simulator, K = %d, 2 iterations' % k,
                   lambda e: policies.CEMGraspPolicy(e, k, num_iterations=2, score='simulator')))
    say('--- %d envs of seed 1005, one reset and one step each (default sigmas %s, decay 0.5, E = K / 4):' % (ne, SIGMAS))
    for name, make in makers:
        e = VecGrasp4DofEnv(ne, seed=1005)
        try:
            obs = e.reset()
            pol = make(e)
            dt = wall(lambda: pol.action(obs))
            a = pol.action(obs)
            extra = ''
            if isinstance(pol, policies.CEMGraspPolicy) and pol.num_iterations:
                par = [p.cpu().numpy() for p in pol.last_choice_parentage[:-1]]
                ne_ = pol.num_elites
                acc = sum(int((p[:, ne_:] >= 0).sum()) for p in par)
                tot = sum(p[:, ne_:].size for p in par)
                sc = [s.cpu().numpy() for s in pol.last_scores]
                ok = (e.antipodal_status == 1).cpu().numpy()
                gain = float(np.mean((sc[-1].max(axis=1) > sc[0].max(axis=1))[ok]))
                extra = '   children accepted %.2f, envs whose best score rose %.2f' % (acc / float(tot), gain)
            _, r, _, _ = e.step(a)
            found = int((e.antipodal_status == 1).sum())
            say('  %-62s success %.3f (%d of %d; %d envs found a grasp)   policy.action %.1f ms%s'
                % (name, float((r > 0).float().mean()), int((r > 0).sum()), ne, found, 1e3 * dt, extra))
        finally:
            e.close()
        flush()


if __name__ == '__main__':
    main()
