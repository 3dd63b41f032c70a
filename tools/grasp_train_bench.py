"""Training the grasp-quality network on the device: what a training step costs next to torch, what six
epochs over a collected set cost and give, and the experiment DESIGN.md 22 asks for -- retraining on refined candidates.

    python tools/grasp_train_bench.py [--iters 20] [--warmup 3] [--envs 2048] [--k 16] [--collect 3] [--epochs 6]
                                      [--eval-envs 1024] [--skip-experiment] [--out profiles/grasp_train_bench.txt]

(a) One training step (forward, BCE-with-logits, backward, Adam) of the default model at m = 256 and m = 2048 on seeded
    crops: ``GraspQualityTrainer.step`` against torch eager on the same device (the same module, loss and
    ``torch.optim.Adam``), alternately, device events, warm-up first, median with min and max of --iters calls each; and the
    three HIP entry points on their own, to say which launch dominates.
(b) --collect calls of ``collect_grasp_samples(K)`` after a reset each (DESIGN.md 21's set), then --epochs epochs of
    ``train(..., backend='hip')``: wall-clock time, held-out loss and accuracy.
(c) With that model: --collect further resets, and per reset ``num_iterations`` rounds of { ``grasp_qualities``;
    ``refine_grasps`` } with CEMGraspPolicy's defaults (E = K / 4, sigmas 3 px / 0.15 rad / 5 mm, decay 0.5); after each
    round the accepted children are cropped and labelled by ``try_grasps``.  The union of (b)'s set and the children is
    trained on afresh (same seed, same epochs), and DESIGN.md 22's table is rerun with both models on --eval-envs envs of
    seed 1005: GraspQualityPolicy, and CEMGraspPolicy with score='model' at 0 to 3 iterations.
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
import torch.nn.functional as F

from robovat_amd import policies
from robovat_amd.envs.grasp.grasp_4dof_env import VecGrasp4DofEnv
from robovat_amd.perception.grasp_quality import GraspQualityModel
from robovat_amd.perception.grasp_quality_trainer import GraspQualityTrainer
from benchlib import alternate

SIGMAS = (3.0, 0.15, 0.005)
DECAY = 0.5
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--k', type=int, default=16)
    ap.add_argument('--collect', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=6)
    ap.add_argument('--eval-envs', type=int, default=1024)
    ap.add_argument('--skip-experiment', action='store_true', help='(a) only')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/grasp_train_bench.py needs a GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    say('tools/grasp_train_bench.py --iters %d --warmup %d --envs %d --k %d --collect %d --epochs %d --eval-envs %d%s on %s'
        % (args.iters, args.warmup, args.envs, args.k, args.collect, args.epochs, args.eval_envs,
           ' --skip-experiment' if args.skip_experiment else '', torch.cuda.get_device_name(0)))
    n, k = args.envs, args.k
    env = VecGrasp4DofEnv(n, seed=5)
    sets, kids = [], []
    try:
        env.reset()
        world = env.world
        # ---- (a) one step
        import grasp_quality_host as gqh
        model = GraspQualityModel.random_init(1, norm=dict(im_mean=0.6, im_inv_std=8.0, z_mean=0.6, z_inv_std=20.0))
        for m in (256, 2048):
            x, z = gqh.sample_inputs(3, m, 32, 32)
            y = (np.random.RandomState(4).uniform(size=m) < 0.3).astype(np.float32)
            xd, zd, yd = (torch.from_numpy(a).to(world.device) for a in (x, z, y))
            trainer = GraspQualityTrainer(world, model)
            net = model.torch_module().to(world.device).train()
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)

            def eager():
                loss = F.binary_cross_entropy_with_logits(net(xd, zd), yd)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss
            logits, ws = world.grasp_quality_forward_train(model, trainer.blob, xd, zd)
            dl = (torch.sigmoid(logits) - yd) / m
            grad = world.grasp_quality_backward(model, trainer.blob, xd, zd, dl, ws)
            blob2, m2, v2 = trainer.blob.clone(), torch.zeros_like(grad), torch.zeros_like(grad)
            fns = {'step': lambda: trainer.step(xd, zd, yd), 'torch': eager,
                   'forward': lambda: world.grasp_quality_forward_train(model, trainer.blob, xd, zd, workspace=ws, out=logits),
                   'backward': lambda: world.grasp_quality_backward(model, trainer.blob, xd, zd, dl, ws, out=grad),
                   'adam': lambda: world.adam_step(blob2, grad, m2, v2, 1)}
            t = alternate(fns, args.iters, args.warmup)
            row = '  %-68s median %8.3f ms   min %8.3f   max %8.3f'
            say('--- (a) one training step of the default model (%d weights), m = %d' % (model.weight_count(), m))
            say(row % (('GraspQualityTrainer.step (4 launches + the loss in torch, incl. the bindings)',) + t['step']))
            say(row % (('torch eager: module forward, BCE, backward, torch.optim.Adam',) + t['torch']))
            say(row % (('  rv_grasp_quality_forward_train alone',) + t['forward']))
            say(row % (('  rv_grasp_quality_backward alone (2 launches)',) + t['backward']))
            say(row % (('  rv_adam_step alone',) + t['adam']))
            say('  torch / HIP step %.2fx' % (t['torch'][0] / t['step'][0]))
        if args.skip_experiment:
            say('--- (b), (c): unmeasured (--skip-experiment)')
            return
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
        x, z, y = (np.concatenate([a[i] for a in sets]) for i in range(3))
        say('  positive share of the labels %.1f %%' % (100.0 * y.mean()))
        spec = importlib.util.spec_from_file_location('train_grasp_quality', os.path.join(HERE, 'train_grasp_quality.py'))
        tool = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(tool)
        t0 = time.perf_counter()
        first, _ = tool.train(x, z, y, epochs=args.epochs, batch=256, lr=1e-3, seed=0, backend='hip', world=world, log=lambda s: say('  ' + s))
        say('  trained %d epochs with backend=\'hip\' in %.1f s (upload and the per-epoch held-out pass included)' % (args.epochs, time.perf_counter() - t0))
        # ---- (c) collect again with refine_grasps in the loop: the children, labelled by try_grasps
        ne = max(1, k // 4)
        t0 = time.perf_counter()
        for i in range(args.collect):
            env.reset()
            depth, _ = world.render()
            env.sample_antipodal_candidates(k, depth=depth)
            for it in range(ROUNDS):
                scores = env.grasp_qualities(first, env.antipodal_image_grasps, depth)
                env.refine_grasps(scores, ne, [s * DECAY ** it for s in SIGMAS], it, depth=depth)
                images, gd = env.grasp_images(env.antipodal_image_grasps, depth)
                r, _ = env.try_grasps(env.antipodal_actions4)
                child = (env.refine_parent >= 0)
                child[:, :ne] = False
                child &= (env.antipodal_status == 1)[:, None] & (env.antipodal_count > 0)[:, None]
                c = child.cpu().numpy()
                kids.append((images.cpu().numpy()[c], gd.cpu().numpy()[c], (r.cpu().numpy()[c] > 0).astype(np.float32), it))
        say('--- (c) %d accepted children of %d refinement rounds per reset labelled by try_grasps in %.1f s' % (sum(len(a[2]) for a in kids), ROUNDS, time.perf_counter() - t0))
        for it in range(ROUNDS):
            yy = np.concatenate([a[2] for a in kids if a[3] == it])
            say('  round %d: %d children, %.1f %% positive' % (it, len(yy), 100.0 * yy.mean()))
        xu, zu, yu = (np.concatenate([x_] + [a[i] for a in kids]) for i, x_ in ((0, x), (1, z), (2, y)))
        t0 = time.perf_counter()
        second, _ = tool.train(xu, zu, yu, epochs=args.epochs, batch=256, lr=1e-3, seed=0, backend='hip', world=world, log=lambda s: say('  ' + s))
        say('  retrained on the union (%d samples, %.1f %% positive) in %.1f s' % (len(yu), 100.0 * yu.mean(), time.perf_counter() - t0))
    finally:
        env.close()
    ev = args.eval_envs
    makers = [('candidate 0 (AntipodalGrasp4DofPolicy)', lambda e: policies.AntipodalGrasp4DofPolicy(e))]
    for tag, mdl in (('first model', first), ('retrained', second)):
        makers.append(('GraspQualityPolicy, K = %d, %s' % (k, tag), lambda e, mdl=mdl: policies.GraspQualityPolicy(e, mdl, k)))
        for its in (0, 1, 2, 3):
            makers.append(('CEMGraspPolicy model, K = %d, %d iteration%s, %s' % (k, its, '' if its == 1 else 's', tag),
                           lambda e, its=its, mdl=mdl: policies.CEMGraspPolicy(e, k, num_iterations=its, model=mdl)))
    say('--- %d envs of seed 1005, one reset and one step each (default sigmas %s, decay %.1f, E = K / 4):' % (ev, SIGMAS, DECAY))
    for name, make in makers:
        e = VecGrasp4DofEnv(ev, seed=1005)
        try:
            obs = e.reset()
            pol = make(e)
            a = pol.action(obs)
            _, r, _, _ = e.step(a)
            say('  %-62s success %.3f (%d of %d)' % (name, float((r > 0).float().mean()), int((r > 0).sum()), ev))
        finally:
            e.close()


if __name__ == '__main__':
    main()
