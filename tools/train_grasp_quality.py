"""Train the grasp-quality network on a labelled grasp set and write it as an .npz that
``GraspQualityModel.load`` reads.

    python tools/train_grasp_quality.py STORE [--out grasp_quality.npz] [--epochs 10] [--batch 256] [--lr 1e-3] [--seed 0]
                                              [--c1 16 --c2 16 --f1 64 --f2 64 --p 16] [--device cpu] [--backend torch|hip]

STORE is a store of ``io.grasp_dataset`` (what ``collect_grasp_samples`` + ``append_grasp_samples`` wrote).  The rows with
``valid`` set are used; the label is ``rewards > 0``; the crop size is the images'.  The normalisation constants are the
mean and 1 / standard deviation of the training pixels and grasp depths.  10 % of the rows (a seeded permutation) are held
out.  Adam on binary cross-entropy with logits over ``GraspQualityModel.torch_module()``; the held-out loss and accuracy
are printed per epoch.  ``--backend hip`` runs the same split, batches, normalisation and initial weights through
``perception.grasp_quality_trainer.GraspQualityTrainer`` instead: forward, backward and Adam as HIP kernels on GPU 0
(DESIGN.md 24), deterministic bit for bit.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from robovat_amd.perception.grasp_quality import GraspQualityModel


def normalisation(images, depths):
    """im_mean, im_inv_std, z_mean, z_inv_std of a training set (float64 statistics, a zero deviation counts as 1)"""
    def inv(s):
        return 1.0 / s if s > 0 and np.isfinite(s) else 1.0
    x, z = np.asarray(images, np.float64), np.asarray(depths, np.float64)
    return {'im_mean': float(x.mean()), 'im_inv_std': inv(float(x.std())), 'z_mean': float(z.mean()), 'z_inv_std': inv(float(z.std()))}


def train(images, depths, labels, epochs=10, batch=256, lr=1e-3, seed=0, holdout=0.1, device='cpu', log=None, backend='torch',
          world=None, **sizes):
    """Train on ``images`` [M, h, w], ``depths`` [M], ``labels`` [M] (0 / 1).  Returns (GraspQualityModel, history) with
    history a list of dicts per epoch: train_loss, holdout_loss, holdout_accuracy (held-out figures NaN when nothing is
    held out).  Deterministic given ``seed`` on the CPU.  ``backend='hip'``: the same split, batches, normalisation and
    initial weights through the HIP trainer on ``world``'s device (any world; None makes a small one on GPU 0);
    deterministic bit for bit; ``device`` is not used."""
    if backend == 'hip':
        return _train_hip(images, depths, labels, epochs, batch, lr, seed, holdout, log, world, sizes)
    if backend != 'torch':
        raise ValueError('train: backend must be \'torch\' or \'hip\', got %r' % (backend,))
    import torch
    import torch.nn.functional as F
    images = np.asarray(images, np.float32)
    depths = np.asarray(depths, np.float32).reshape(-1)
    labels = np.asarray(labels, np.float32).reshape(-1)
    m = len(images)
    rng = np.random.RandomState(seed)
    order = rng.permutation(m)
    n_hold = int(round(holdout * m))
    hold, tr = order[:n_hold], order[n_hold:]
    norm = normalisation(images[tr], depths[tr])
    sizes = dict(sizes, height=images.shape[1], width=images.shape[2])
    model = GraspQualityModel.random_init(seed, norm=norm, **sizes)
    torch.manual_seed(seed)
    net = model.torch_module().to(device)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    x, z, y = (torch.from_numpy(a).to(device) for a in (images, depths, labels))
    history = []
    for epoch in range(epochs):
        net.train()
        perm = rng.permutation(tr)
        total = 0.0
        for i in range(0, len(perm), batch):
            idx = torch.from_numpy(perm[i:i + batch]).to(device)
            loss = F.binary_cross_entropy_with_logits(net(x[idx], z[idx]), y[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += float(loss.detach()) * len(idx)
        row = {'train_loss': total / max(len(perm), 1), 'holdout_loss': float('nan'), 'holdout_accuracy': float('nan')}
        if n_hold:
            net.eval()
            with torch.no_grad():
                hi = torch.from_numpy(hold).to(device)
                logit = net(x[hi], z[hi])
                row['holdout_loss'] = float(F.binary_cross_entropy_with_logits(logit, y[hi]))
                row['holdout_accuracy'] = float(((logit > 0).float() == y[hi]).float().mean())
        history.append(row)
        if log:
            log('epoch %3d  train loss %.4f  held-out loss %.4f  held-out accuracy %.3f'
                % (epoch, row['train_loss'], row['holdout_loss'], row['holdout_accuracy']))
    return GraspQualityModel.from_torch_module(net.cpu()), history


def _train_hip(images, depths, labels, epochs, batch, lr, seed, holdout, log, world, sizes):
    import torch
    import torch.nn.functional as F
    from robovat_amd.perception.grasp_quality_trainer import GraspQualityTrainer
    from robovat_amd import abi
    if not 1 <= batch <= abi.RV_GQ_MAX_BATCH:
        raise ValueError('train: batch outside [1, %d]' % abi.RV_GQ_MAX_BATCH)
    images = np.asarray(images, np.float32)
    depths = np.asarray(depths, np.float32).reshape(-1)
    labels = np.asarray(labels, np.float32).reshape(-1)
    m = len(images)
    rng = np.random.RandomState(seed)
    order = rng.permutation(m)
    n_hold = int(round(holdout * m))
    hold, tr = order[:n_hold], order[n_hold:]
    norm = normalisation(images[tr], depths[tr])
    sizes = dict(sizes, height=images.shape[1], width=images.shape[2])
    model = GraspQualityModel.random_init(seed, norm=norm, **sizes)
    own = world is None
    if own:
        from robovat_amd import configs, lib, scenes
        scene, names = scenes.make_scene()
        world = lib.World(configs.make_rv_config(n_envs=1, shape_names=names), scene, device=0)
    try:
        trainer = GraspQualityTrainer(world, model, lr=lr)
        x, z, y = trainer.load_data(images, depths, labels)
        history = []
        for epoch in range(epochs):
            perm = rng.permutation(tr)
            total = torch.zeros((), dtype=torch.float64, device=world.device)
            for i in range(0, len(perm), batch):
                idx = perm[i:i + batch]
                total = total + trainer.step_indices(idx).double() * len(idx)
            row = {'train_loss': float(total) / max(len(perm), 1), 'holdout_loss': float('nan'), 'holdout_accuracy': float('nan')}
            if n_hold:
                hi = torch.from_numpy(hold).to(world.device)
                logit = torch.cat([trainer.logits(x[hi[i:i + abi.RV_GQ_MAX_BATCH]], z[hi[i:i + abi.RV_GQ_MAX_BATCH]])
                                   for i in range(0, n_hold, abi.RV_GQ_MAX_BATCH)])
                row['holdout_loss'] = float(F.binary_cross_entropy_with_logits(logit, y[hi]))
                row['holdout_accuracy'] = float(((logit > 0).float() == y[hi]).float().mean())
            history.append(row)
            if log:
                log('epoch %3d  train loss %.4f  held-out loss %.4f  held-out accuracy %.3f'
                    % (epoch, row['train_loss'], row['holdout_loss'], row['holdout_accuracy']))
        return trainer.model(), history
    finally:
        if own:
            world.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('store')
    ap.add_argument('--out', default='grasp_quality.npz')
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cpu')
    ap.add_argument('--backend', default='torch', choices=('torch', 'hip'))
    for name, default in (('c1', 16), ('c2', 16), ('f1', 64), ('f2', 64), ('p', 16)):
        ap.add_argument('--' + name, type=int, default=default)
    args = ap.parse_args()
    from robovat_amd.io import grasp_dataset, hdf5_utils
    with hdf5_utils.open_store(args.store, 'r') as store:
        data = grasp_dataset.read_grasp_samples(store)
    keep = np.asarray(data['valid'], bool)
    images, depths = data['images'][keep], data['grasp_depths'][keep]
    labels = (data['rewards'][keep] > 0).astype(np.float32)
    print('%d valid samples of %d, %.1f %% positive, crops %d x %d' % (keep.sum(), len(keep), 100.0 * labels.mean(), images.shape[1], images.shape[2]))
    model, _ = train(images, depths, labels, epochs=args.epochs, batch=args.batch, lr=args.lr, seed=args.seed, device=args.device,
                     backend=args.backend, log=print, c1=args.c1, c2=args.c2, f1=args.f1, f2=args.f2, p=args.p)
    model.save(args.out)
    print('wrote %s (%d weights)' % (args.out, model.weight_count()))


if __name__ == '__main__':
    main()
