"""Generate tests/golden/depth_noise_golden.json by RUNNING the reference's perception/depth_utils.py (build container
only).

    python tests/golden/gen_depth_noise_golden.py

gen_golden.py is imported for the stubs it installs (pybullet, cv2, gym, easydict, the numpy-1 names).  On top of them:
a shim for the removed ``scipy.misc.imresize`` that does what the old one did for mode='F' (Pillow fromarray ->
resize(BICUBIC) -> array), and patches that make ``scipy.stats.gamma.rvs``, ``scipy.stats.norm.rvs`` and
``np.random.rand`` return the values tests/depth_noise_host.py draws, so that the reference and the restatement consume
the same randomness.  Only DATA is written: the inputs, the supplied draws and the reference's outputs.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden  # noqa: E402,F401  (the stubs)
import scipy.misc  # noqa: E402
import scipy.stats  # noqa: E402
import PIL.Image  # noqa: E402

import depth_noise_host as dnh  # noqa: E402


def imresize(arr, size, interp='bilinear', mode=None):
    """scipy.misc.imresize as it was (scipy 1.2), for a float image and a scale factor"""
    assert mode == 'F' and interp == 'bicubic' and isinstance(size, float)
    im = PIL.Image.fromarray(np.asarray(arr, np.float32))
    assert im.mode == 'F'
    new = tuple((np.array(im.size) * size).astype(int))
    return np.array(im.resize(new, resample=PIL.Image.BICUBIC))


scipy.misc.imresize = imresize

from robovat.perception import depth_utils  # noqa: E402

F = np.float32
SEED_LO, SEED_HI = 0x9e3779b9, 0x7f4a7c15
CASES = [
    # height, width, R, gids, seed, draw_index, gamma_shape, prob, sigma
    (8, 12, 4, [5, 6, 7], 3, 0, 1000.0, 0.5, 0.005),
    (24, 32, 4, [5, 6, 7], 4, 1, 1000.0, 0.5, 0.005),
    (10, 14, 2, [5, 6, 7], 9, 77, 2.0, 0.5, 0.01),
    (6, 6, 1, [5, 6, 7], 6, (1 << 24) - 1, 50.0, 0.5, 0.02),
]
THRESHOLD_MARGIN = 1e-5


def f32_list(a):
    """float32 values as the shortest decimals that read back to the same float32"""
    return [float(str(v)) for v in np.asarray(a, F).reshape(-1)]


def depth_images(rng, n, height, width):
    """a table at 0.7 m with a slanted box and smooth relief on it, scattered zero pixels (nothing hit)"""
    y, x = np.mgrid[0:height, 0:width]
    out = []
    for i in range(n):
        d = 0.7 + 0.01 * np.sin(0.9 * x + i) * np.cos(0.7 * y) + 0.002 * rng.standard_normal((height, width))
        box = (np.abs(x - width / 2.0) < width / 4.0) & (np.abs(y - height / 2.0) < height / 4.0)
        d = np.where(box, d - 0.05 - 0.004 * x, d)
        d[rng.random((height, width)) < 0.12] = 0.0
        out.append(d)
    return np.stack(out).astype(F)


def pick_threshold(image):
    """a threshold in the widest gap of the middle half of the image's float64 gradient magnitudes"""
    g0, g1 = np.gradient(np.asarray(image, F))
    mag = np.sort(np.sqrt(g0.astype(np.float64) ** 2 + g1.astype(np.float64) ** 2).reshape(-1))
    lo, hi = len(mag) // 4, 3 * len(mag) // 4
    k = lo + int(np.argmax(np.diff(mag[lo:hi])))
    thr = float(F(0.5 * (mag[k] + mag[k + 1])))
    assert np.all(np.abs(mag - thr) > THRESHOLD_MARGIN * thr), 'a gradient magnitude next to the threshold'
    return thr


def main():
    rng = np.random.default_rng(20260119)
    cases = []
    for height, width, R, gids, seed, draw_index, shape, prob, sigma in CASES:
        p = {'height': height, 'width': width, 'draw_index': draw_index, 'seed': seed, 'gamma_shape': shape,
             'prob': prob, 'rescale_factor': R, 'sigma': sigma}
        n = len(gids)
        depth = depth_images(rng, n, height, width)
        assert np.any(depth == 0)
        drawn = [dnh.draws(SEED_LO, SEED_HI, gid, p) for gid in gids]
        g = np.array([d[0] for d in drawn], F)
        applied = [d[1] for d in drawn]
        grid = np.stack([d[2] for d in drawn])
        # the uniform behind `applied`, and the grid the reference would draw for an env the kernel skips
        rand = [float(F(int(dnh.block(SEED_LO, SEED_HI, np.array([gid], np.uint64), p, np.array([dnh.SCALAR_BLOCK], np.uint64))[3][0]) >> 8)
                      * dnh.TWO_M24) for gid in gids]
        assert [int(u < prob) for u in rand] == applied
        assert set(applied) == {0, 1}, 'every case holds applied and skipped envs'
        state = {'i': -1}

        def gamma_rvs(a, scale=1.0, size=None):
            assert a == shape and scale == 1.0 / shape and size == n
            return g.astype(np.float64)

        def rand_fn():
            state['i'] += 1
            return rand[state['i']]

        def norm_rvs(scale=1.0, size=None):
            assert scale == sigma and size == (height // R) * (width // R) and applied[state['i']]
            return grid[state['i']].astype(np.float64).reshape(-1)

        keep = scipy.stats.gamma.rvs, scipy.stats.norm.rvs, np.random.rand
        scipy.stats.gamma.rvs, scipy.stats.norm.rvs, np.random.rand = gamma_rvs, norm_rvs, rand_fn
        try:
            gamma_out = depth_utils.gamma_noise(depth[..., None].copy(), gamma_shape=shape)
            gauss_out = depth_utils.gaussian_noise(gamma_out.copy(), prob=prob, rescale_factor=float(R), sigma=sigma)
            state['i'] = -1
            gauss_f32 = depth_utils.gaussian_noise(gamma_out.astype(F), prob=prob, rescale_factor=float(R), sigma=sigma)
        finally:
            scipy.stats.gamma.rvs, scipy.stats.norm.rvs, np.random.rand = keep
        assert gamma_out.dtype == np.float64 and gauss_out.dtype == np.float64 and gauss_f32.dtype == F
        thr = pick_threshold(depth[0])
        thr_out = depth_utils.threshold_gradients(depth[0], thr)
        assert 0 < np.count_nonzero((thr_out == 0) & (depth[0] != 0)) < depth[0].size
        cases.append({
            'params': p, 'seed_lo': SEED_LO, 'seed_hi': SEED_HI, 'gids': gids,
            'depth': f32_list(depth), 'g': f32_list(g), 'rand': rand, 'applied': applied, 'grid': f32_list(grid),
            'gamma_out': gamma_out.reshape(-1).tolist(), 'gauss_out': gauss_out.reshape(-1).tolist(),
            'gauss_out_f32': f32_list(gauss_f32),
            'threshold': thr, 'threshold_out': f32_list(thr_out),
        })
    with open(os.path.join(HERE, 'depth_noise_golden.json'), 'w') as f:
        json.dump({'cases': cases}, f, sort_keys=True, separators=(',', ':'))
        f.write('\n')


if __name__ == '__main__':
    main()
