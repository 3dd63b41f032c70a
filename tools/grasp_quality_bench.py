"""The grasp-quality network on the device: what rv_grasp_quality costs at the product's shape, and what a
network trained on a collected set is worth as a ranking.

    python tools/grasp_quality_bench.py [--envs 2048] [--k 16] [--iters 20] [--warmup 3] [--skip-policy]
                                        [--collect 3] [--epochs 6] [--eval-envs 1024] [--out profiles/grasp_quality_bench.txt]

(a) N config-4 grasp envs are reset and rendered once, rv_policy_antipodal_multi gives K image grasps per env and
    rv_grasp_crops their 32 x 32 crops; rv_grasp_quality with a seeded default model (73 617 weights) is timed on them
    against the eager float32 forward of ``GraspQualityModel.torch_module()`` on the same device -- alternately, device
    events, warm-up first, median with min and max of --iters calls each -- and against the time its FLOP would take at the
    157.3 TF f32 matrix peak.  The logits of a 256-crop slice are compared bit for bit with tests/grasp_quality_host.py.
(b) --collect calls of ``collect_grasp_samples(K)`` after a reset each give a labelled set; tools/train_grasp_quality.py's
    ``train`` fits the default model to it on the CPU; then on --eval-envs envs of another seed, one step after one reset
    each (the same scenes for every policy), the share of envs whose grasp earns a positive reward under candidate 0
    (AntipodalGrasp4DofPolicy), GraspQualityPolicy at K and LookaheadGrasp4DofPolicy at K (the ceiling: it executes all K),
    and the wall-clock time of one ``policy.action`` each.
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

from robovat_amd import lib, policies
from robovat_amd.envs.grasp.grasp_4dof_env import VecGrasp4DofEnv
from robovat_amd.perception.grasp_quality import GraspQualityModel
from benchlib import alternate, wall

PEAK_F32_MATRIX_TF = 157.3


def flop_per_crop(s):
    h, w = s['height'], s['width']
    k1 = s['c2'] * (h // 4) * (w // 4)
    return 2.0 * (25 * s['c1'] * h * w + 9 * s['c1'] * s['c2'] * (h // 2) * (w // 2) + k1 * s['f1'] + s['p']
                  + (s['f1'] + s['p']) * s['f2'] + s['f2'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--collect', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--skip-policy', action='store_true', help='the kernel half only (a profiler run)')
    ap.add_argument('--skip-torch', action='store_true', help='no eager torch forward next to the kernel')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/grasp_quality_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('tools/grasp_quality_bench.py --envs %d --k %d --iters %d --warmup %d --collect %d --epochs %d --eval-envs %d%s on %s'
        % (args.envs, args.k, args.iters, args.warmup, args.collect, args.epochs, args.eval_envs,
           ' --skip-policy' if args.skip_policy else '', torch.cuda.get_device_name(0)))
    n, k = args.envs, args.k
    env = VecGrasp4DofEnv(n, seed=5)
    sets = []
    try:
        env.reset()
        world = env.world
        depth, _ = world.render()
        env.sample_antipodal_candidates(k, depth=depth)
        images, gd = env.grasp_images(depth=depth)
        model = GraspQualityModel.random_init(1, norm=dict(im_mean=0.6, im_inv_std=8.0, z_mean=0.6, z_inv_std=20.0))
        out = world.grasp_quality(images, gd, model)
        torch.cuda.synchronize()
        # ---- (a) the kernel
        import grasp_quality_host as gqh
        flat = images.reshape((n * k,) + tuple(images.shape[2:]))
        sl = slice(0, min(256, n * k))
        host = gqh.forward(model.params, model.norm, flat[sl].cpu().numpy(), gd.reshape(-1)[sl].cpu().numpy())
        got = out.reshape(-1)[sl].cpu().numpy()
        differ = int((got.view(np.uint32) != host.view(np.uint32)).sum())
        say('--- (a) %d x %d crops of 32 x 32, default model (%d weights): %d of %d logits of a slice differ from the float32 restatement'
            % (n, k, model.weight_count(), differ, got.size))
        fns = {'kernel': lambda: world.grasp_quality(images, gd, model, out=out)}
        if not args.skip_torch:
            net = model.torch_module().to(world.device).eval()
            zf = gd.reshape(-1)

            def eager():
                with torch.no_grad():
                    return net(flat, zf)
            ref = eager()
            torch.cuda.synchronize()
            dmax = float((ref - out.reshape(-1)).abs().max())
            say('  largest |kernel - torch eager| over all logits %.3e (another summation order)' % dmax)
            fns['torch'] = eager
        t = alternate(fns, args.iters, args.warmup)
        gflop = flop_per_crop(model.sizes) * n * k / 1e9
        ideal = gflop / PEAK_F32_MATRIX_TF      # ms: GFLOP / (TFLOP/s) = ms
        row = '  %-58s median %8.3f ms   min %8.3f   max %8.3f'
        say(row % (('rv_grasp_quality (one launch, incl. the binding)',) + t['kernel']))
        if 'torch' in t:
            say(row % (('torch eager float32 forward of torch_module()',) + t['torch']))
            say('  torch / kernel %.2fx' % (t['torch'][0] / t['kernel'][0]))
        say('  %.1f GFLOP per call; at the %.1f TF f32 matrix peak %.3f ms; achieved %.1f TF = %.1f %% of peak'
            % (gflop, PEAK_F32_MATRIX_TF, ideal, gflop / t['kernel'][0], 100.0 * ideal / t['kernel'][0]))
        if args.skip_policy:
            say('--- (b) ranking: unmeasured (--skip-policy)')
        else:
            # ---- (b) collect
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
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    x, z, y = (np.concatenate([a[i] for a in sets]) for i in range(3))
    say('  positive share of the labels %.1f %%' % (100.0 * y.mean()))
    spec = importlib.util.spec_from_file_location('train_grasp_quality', os.path.join(HERE, 'train_grasp_quality.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t0 = time.perf_counter()
    trained, history = tool.train(x, z, y, epochs=args.epochs, batch=256, lr=1e-3, seed=0, log=lambda s: say('  ' + s))
    say('  trained %d epochs on the CPU in %.1f s' % (args.epochs, time.perf_counter() - t0))
    # ---- evaluate: the same scenes for every policy (a fresh env of one seed each)
    ne = args.eval_envs
    makers = (('candidate 0 (AntipodalGrasp4DofPolicy)', lambda e: policies.AntipodalGrasp4DofPolicy(e)),
              ('GraspQualityPolicy, K = %d, trained model' % k, lambda e: policies.GraspQualityPolicy(e, trained, k)),
              ('GraspQualityPolicy, K = %d, untrained model (seed 1)' % k, lambda e: policies.GraspQualityPolicy(e, model, k)),
              ('LookaheadGrasp4DofPolicy, K = %d (executes all K)' % k, lambda e: policies.LookaheadGrasp4DofPolicy(e, k)))
    say('--- %d envs of seed 1005, one reset and one step each:' % ne)
    for name, make in makers:
        e = VecGrasp4DofEnv(ne, seed=1005)
        try:
            obs = e.reset()
            pol = make(e)
            dt = wall(lambda: pol.action(obs))
            a = pol.action(obs)
            _, r, _, _ = e.step(a)
            found = int((e.antipodal_status == 1).sum())
            say('  %-58s success %.3f (%d of %d; %d envs found a grasp)   policy.action %.1f ms'
                % (name, float((r > 0).float().mean()), int((r > 0).sum()), ne, found, 1e3 * dt))
        finally:
            e.close()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
