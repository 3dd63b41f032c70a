"""Labelled grasp samples on disk: what ``VecGrasp4DofEnv.collect_grasp_samples`` returns, one row per candidate.

A store of ``hdf5_utils.open_store`` (an ``h5py.File``, or the ``.npz`` tree where h5py is absent) gets one group per
append, ``grasp_samples_000000``, ``grasp_samples_000001``, ..., each holding arrays whose first axis is the sample:

    images [M, h, w] float32        the grasp-centred depth crop (rv_grasp_crops)
    grasp_depths [M] float32        the depth of the grasp (column 4 of its image grasp)
    image_grasps [M, 5] float32     x1, y1, x2, y2, depth in the depth image
    actions4 [M, 4] float32         the world action that was tried
    rewards [M] float32, dones [M] uint8      GraspReward of the trial
    valid [M] bool                  a grasp the sampler found (not a repeated row, not a random draw)
    env [M], candidate [M] int32    where the row stood in the [N, K] batch of its append

``read_grasp_samples`` gives the arrays back concatenated over the appends, in append order.
"""
import numpy as np

from robovat_amd.io import hdf5_utils

PREFIX = 'grasp_samples_'
PER_SAMPLE = ('images', 'grasp_depths', 'image_grasps', 'actions4', 'rewards', 'dones', 'valid')
KEYS = PER_SAMPLE + ('env', 'candidate')


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def _groups(store):
    return sorted(k for k, _ in store.items() if k.startswith(PREFIX))


def append_grasp_samples(store, samples, only_valid=True):
    """Append the [N, K] batch ``samples`` (the dict of ``collect_grasp_samples``; tensors or arrays, with or without the
    env axis) to ``store`` as one group of M rows: those with ``valid`` set, or all N K with ``only_valid=False``.
    Returns the group's name."""
    valid = _np(samples['valid']).astype(bool)
    if valid.ndim == 1:
        valid = valid[None]
    n, k = valid.shape
    rows = {}
    for key in PER_SAMPLE:
        a = _np(samples[key])
        if a.shape[:2] != (n, k):
            a = a[None]
        if a.shape[:2] != (n, k):
            raise ValueError('append_grasp_samples: %s must be [N, K, ...] = [%d, %d, ...], got %s' % (key, n, k, a.shape))
        rows[key] = a.reshape((n * k,) + a.shape[2:])
    rows['env'] = np.repeat(np.arange(n, dtype=np.int32), k)
    rows['candidate'] = np.tile(np.arange(k, dtype=np.int32), n)
    if only_valid:
        keep = valid.reshape(-1)
        rows = {key: a[keep] for key, a in rows.items()}
    name = '%s%06d' % (PREFIX, len(_groups(store)))
    hdf5_utils.write_data_to_hdf5(store.create_group(name), rows)
    return name


def read_grasp_samples(store):
    """The arrays of every append of ``store``, concatenated along the sample axis in append order: a dict with the keys
    of ``KEYS`` (empty dict for a store without samples)."""
    parts = [hdf5_utils.read_data_from_hdf5(dict(store.items())[name]) for name in _groups(store)]
    if not parts:
        return {}
    return {key: np.concatenate([np.asarray(p[key]) for p in parts], axis=0) for key in KEYS}
