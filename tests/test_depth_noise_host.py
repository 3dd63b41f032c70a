"""The depth sensor noise model (csrc/rv_dev_depth_noise.h) on the CPU, through its NumPy restatement
tests/depth_noise_host.py (the GPU tests pin the kernels to that restatement bit for bit) and the host mirrors of
robovat_amd/perception/depth_utils.py: against what the reference itself computed from the same draws
(golden/depth_noise_golden.json, written by golden/gen_depth_noise_golden.py), against Pillow, against scipy's gamma
distribution and against float64."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import depth_noise_host as host
from cem_host import logr

F = np.float32
U = 2.0 ** -24      # the unit roundoff of float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEED_LO, SEED_HI = 0x1234abcd, 0x0badcafe
SHAPES = [(8, 12, 4), (24, 32, 4), (10, 14, 2), (6, 6, 1)]      # (H, W, R) of the golden's cases


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _params(height=8, width=12, R=4, draw_index=0, seed=0, gamma_shape=1000.0, prob=0.5, sigma=0.005):
    return {'height': height, 'width': width, 'draw_index': draw_index, 'seed': seed, 'gamma_shape': gamma_shape,
            'prob': prob, 'rescale_factor': R, 'sigma': sigma}


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F)).astype(np.float64)


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(HERE, 'golden', 'depth_noise_golden.json')) as f:
        cases = json.load(f)['cases']
    out = []
    for c in cases:
        p = c['params']
        n, H, W, R = len(c['gids']), p['height'], p['width'], p['rescale_factor']
        d = dict(c)
        d['depth'] = np.array(c['depth'], F).reshape(n, H, W)
        d['g'] = np.array(c['g'], F)
        d['grid'] = np.array(c['grid'], F).reshape(n, H // R, W // R)
        d['gamma_out'] = np.array(c['gamma_out'], np.float64).reshape(n, H, W)
        d['gauss_out'] = np.array(c['gauss_out'], np.float64).reshape(n, H, W)
        d['gauss_out_f32'] = np.array(c['gauss_out_f32'], F).reshape(n, H, W)
        d['threshold_out'] = np.array(c['threshold_out'], F).reshape(H, W)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(d)
    assert [(c['params']['height'], c['params']['width'], c['params']['rescale_factor']) for c in out] == SHAPES
    return out


# ---- the golden: the reference's own functions fed with the restatement's draws
def test_golden_draws_are_the_restatements(golden):
    """the draws the generator supplied to the reference are what ``draws`` gives today"""
    for c in golden:
        for i, gid in enumerate(c['gids']):
            g, applied, grid = host.draws(c['seed_lo'], c['seed_hi'], gid, c['params'])
            assert _same(g, c['g'][i]) and applied == c['applied'][i] and _same(grid, c['grid'][i])
        assert set(c['applied']) == {0, 1}


def test_apply_against_the_reference(golden):
    """``apply`` against gamma_noise followed by gaussian_noise of the reference (float64 image, Pillow's resize).
    The gamma product: within 1 ulp of the reference's float64 product.  The bicubic sum: within B = 16 * 2^-24 *
    max|grid| of Pillow's (two passes of at most four rounded multiply-adds each, tap gain at most 1.25 per pass).  The
    whole: the product's rounding (1/2 ulp) + B + the final sum's rounding (1/2 ulp).  Zero pixels stay exactly zero; an
    env the noise is not applied to carries the gamma product alone.  Measured: product 0.50 ulp, bicubic sum 0.23 B at
    worst (the 6 x 6, R = 1 case is exact)."""
    worst_prod = worst_up = 0.0
    for c in golden:
        R = c['params']['rescale_factor']
        out = host.apply(c['depth'], c['g'], c['applied'], c['grid'], R)
        assert out.dtype == F
        prod = host.apply(c['depth'], c['g'], np.zeros(len(c['gids']), np.uint8), c['grid'], R)
        err = np.abs(prod.astype(np.float64) - c['gamma_out'])
        assert np.all(err <= _ulp32(c['gamma_out']))
        worst_prod = max(worst_prod, float((err / _ulp32(c['gamma_out']))[c['gamma_out'] != 0].max()))
        zero = c['depth'] == 0
        assert zero.any() and np.all(_bits(out[zero]) == 0) and np.all(c['gauss_out'][zero] == 0)
        B = 16.0 * U * float(np.abs(c['grid']).max())
        up_ref = c['gauss_out'] - c['gamma_out']            # (float64: Pillow's float32 noise, to 1e-16)
        up = host.upsample(c['grid'], R).astype(np.float64)
        for i, applied in enumerate(c['applied']):
            if not applied:
                assert _same(out[i], prod[i]) and np.array_equal(c['gauss_out'][i], c['gamma_out'][i])
                continue
            hit = ~zero[i]
            e = np.abs(up[i] - up_ref[i])[hit]
            assert np.all(e <= B + 1e-15), (c['params'], e.max(), B)
            worst_up = max(worst_up, float(e.max() / B))
        tol = 0.5 * _ulp32(c['gamma_out']) + B + 0.5 * _ulp32(c['gauss_out']) + 1e-15
        assert np.all(np.abs(out.astype(np.float64) - c['gauss_out']) <= tol)
    print('apply: gamma product %.2f ulp, bicubic sum %.3f of its bound at worst' % (worst_prod, worst_up))


def _patched(monkeypatch, c):
    """NumPy's global generator replaced by the golden's supplied draws, in the order the mirrors ask for them"""
    state = {'i': -1}
    n = len(c['gids'])

    def gamma(shape, scale=1.0, size=None):
        assert shape == c['params']['gamma_shape'] and size == n
        return c['g'].astype(np.float64)

    def rand():
        state['i'] += 1
        return c['rand'][state['i']]

    def normal(loc=0.0, scale=1.0, size=None):
        assert scale == c['params']['sigma'] and c['applied'][state['i']]
        return c['grid'][state['i']].astype(np.float64).reshape(-1)

    monkeypatch.setattr(np.random, 'gamma', gamma)
    monkeypatch.setattr(np.random, 'rand', rand)
    monkeypatch.setattr(np.random, 'normal', normal)
    return state


def test_host_mirrors_against_the_reference(golden, monkeypatch):
    """perception.depth_utils with the golden's draws: gamma_noise equals the reference's float64 product exactly,
    gaussian_noise lies within the bicubic bound of it (float64 and float32 images), threshold_gradients zeroes the same
    pixels -- no pixel excluded (the generator keeps every gradient magnitude 1e-5 relative away from the threshold)."""
    from robovat_amd.perception import depth_utils
    for c in golden:
        p = c['params']
        state = _patched(monkeypatch, c)
        data = c['depth'][..., None].copy()
        gamma_out = depth_utils.gamma_noise(data, gamma_shape=p['gamma_shape'])
        assert gamma_out.dtype == np.float64 and np.array_equal(gamma_out[..., 0], c['gamma_out'])
        assert np.array_equal(data[..., 0], c['depth'])
        B = 16.0 * U * float(np.abs(c['grid']).max())
        kept = gamma_out.copy()
        out = depth_utils.gaussian_noise(gamma_out, prob=p['prob'], rescale_factor=float(p['rescale_factor']), sigma=p['sigma'])
        assert out.shape == gamma_out.shape and out.dtype == np.float64 and np.array_equal(gamma_out, kept)
        assert np.all(np.abs(out[..., 0] - c['gauss_out']) <= B + 1e-15)
        state['i'] = -1
        out32 = depth_utils.gaussian_noise(gamma_out.astype(F), prob=p['prob'], rescale_factor=float(p['rescale_factor']), sigma=p['sigma'])
        assert out32.dtype == F
        assert np.all(np.abs(out32[..., 0].astype(np.float64) - c['gauss_out_f32']) <= B + _ulp32(c['gauss_out_f32']))
        # a single image [H, W, C] goes through the same path
        state['i'] = -1
        one = depth_utils.gaussian_noise(gamma_out[0], prob=p['prob'], rescale_factor=p['rescale_factor'], sigma=p['sigma'])
        assert np.array_equal(one, out[0])
        thr = depth_utils.threshold_gradients(c['depth'][0], c['threshold'])
        assert _same(thr, c['threshold_out'])
        assert 0 < np.count_nonzero((thr == 0) & (c['depth'][0] != 0))


def test_mirrors_refuse_what_the_reference_breaks_on():
    from robovat_amd.perception import depth_utils
    img = np.ones((8, 12, 1), F)
    with pytest.raises(ValueError):
        depth_utils.gaussian_noise(img, rescale_factor=5.0)
    with pytest.raises(ValueError):
        depth_utils.gaussian_noise(img, rescale_factor=2.5)
    with pytest.raises(ValueError):
        depth_utils.resize_bicubic(np.ones((2, 2), F), 1.5)
    assert not hasattr(depth_utils, 'inpaint')


# ---- the resize against Pillow itself
@pytest.mark.parametrize('h,w,R', [(2, 3, 4), (6, 8, 4), (3, 5, 3), (5, 7, 2), (2, 2, 4), (6, 6, 1), (4, 4, 8), (106, 128, 4)])
def test_resize_bicubic_against_pillow(h, w, R):
    """resize_bicubic, and the restatement's upsample (bit for bit the same), against Image.resize(BICUBIC) of a mode-F
    image on N(0, 0.005^2) grids: within 16 * 2^-24 * max|grid| (measured: 3.7e-9 at 106 x 128, about 2 ulp of the largest
    value)."""
    from PIL import Image
    from robovat_amd.perception import depth_utils
    grid = (0.005 * np.random.default_rng(h * 1000 + w * 10 + R).standard_normal((h, w))).astype(F)
    got = depth_utils.resize_bicubic(grid, R)
    assert got.shape == (h * R, w * R) and got.dtype == F
    assert _same(got, host.upsample(grid, R))
    want = np.array(Image.fromarray(grid).resize((w * R, h * R), resample=Image.BICUBIC))
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print('resize %d x %d x %d: max |difference from Pillow| %.2e (bound %.2e)' % (h, w, R, err, 16 * U * np.abs(grid).max()))
    assert err <= 16.0 * U * float(np.abs(grid).max())


def test_taps_are_pillows():
    """2 or 3 taps at a border, 4 inside, each set normalised; R distinct interior weight sets for a power of two; R = 1 is
    the identity"""
    for R in range(1, 9):
        lo, nt, w = host.taps(12 * R, R, 12)
        assert nt.min() >= 2 and nt.max() == 4 and np.all(lo >= 0) and np.all(lo + nt <= 12)
        assert np.all(np.abs(w.astype(np.float64).sum(axis=1) - 1.0) <= 4 * U)
        inside = nt == 4
        if R in (1, 2, 4, 8):      # (centre and offsets are exact in float32: the sets repeat bit for bit)
            assert len({tuple(_bits(row)) for row in w[inside]}) <= R
        assert nt[0] < 4 and nt[-1] < 4
    x = np.random.default_rng(0).standard_normal((6, 6)).astype(F)
    assert _same(host.upsample(x, 1), x)


# ---- the draws
@pytest.fixture(scope='module')
def multipliers():
    """2^16 gamma multipliers per shape k: 4096 env ids x 16 draw indices -> {k: (g, attempts used)}"""
    out = {}
    gid = np.arange(4096, dtype=np.uint64)
    for k in (1000.0, 2.0):
        parts = [host.scalars(SEED_LO, SEED_HI, gid, _params(draw_index=di, gamma_shape=k))
                 for di in list(range(8)) + [1000 + 37 * i for i in range(8)]]
        g = np.concatenate([pt[0] for pt in parts])
        used = np.concatenate([pt[2] for pt in parts])
        assert g.size == 1 << 16 and g.dtype == F
        out[k] = (g, used)
    return out


@pytest.mark.parametrize('k', [1000.0, 2.0])
def test_gamma_multipliers_follow_the_distribution(multipliers, k):
    """The empirical CDF of 2^16 multipliers within the DKW bound sqrt(ln(2 / 1e-6) / (2 n)) = 0.0105 of Gamma(k, 1 / k);
    the mean within 5 standard errors of 1; no draw took the four-rejection fallback."""
    from scipy import stats
    g, used = multipliers[k]
    n = g.size
    x = np.sort(g.astype(np.float64))
    cdf = stats.gamma(k, scale=1.0 / k).cdf(x)
    d = max(np.abs(cdf - np.arange(1, n + 1) / n).max(), np.abs(cdf - np.arange(0, n) / n).max())
    bound = np.sqrt(np.log(2.0 / 1e-6) / (2.0 * n))
    se = np.sqrt(1.0 / k / n)
    print('gamma k = %g: sup |F_n - F| = %.4f (bound %.4f), mean - 1 = %.2e (5 se = %.2e), attempts used %s'
          % (k, d, bound, x.mean() - 1, 5 * se, np.bincount(used, minlength=5).tolist()))
    assert abs(bound - 0.0105) < 1e-4 and d <= bound
    assert abs(x.mean() - 1.0) <= 5.0 * se
    assert np.all(used < 4) and np.all(g > 0)
    assert used.max() >= 1      # (rejections do happen: the later attempts are exercised)


def test_gamma_off_draws_nothing_and_gives_one():
    g, applied, used = host.scalars(SEED_LO, SEED_HI, np.arange(64), _params(gamma_shape=0.0))
    assert np.all(_bits(g) == _bits(F(1.0))) and np.all(used == 0)
    g2, applied2, _ = host.scalars(SEED_LO, SEED_HI, np.arange(64), _params(gamma_shape=1000.0))
    assert np.array_equal(applied, applied2)      # (the flag does not depend on the gamma draw)


def test_grid_normals_mean_and_variance():
    p = _params(height=424, width=512, R=4, prob=1.0, sigma=0.005)
    g, applied, grid = host.draws(SEED_LO, SEED_HI, 3, p)
    assert applied == 1 and grid.shape == (106, 128)
    z = grid.astype(np.float64).ravel() / 0.005
    n = z.size
    print('grid: mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)' % (z.mean(), 5 / np.sqrt(n), z.var() - 1, 5 * np.sqrt(2.0 / n)))
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert _same(grid, (F(0.005) * host.grid_normals(SEED_LO, SEED_HI, 3, p, 106 * 128)).reshape(106, 128))


@pytest.mark.parametrize('prob', [0.5, 0.1])
def test_applied_rate(prob):
    n = 1 << 16
    _, applied, _ = host.scalars(SEED_LO, SEED_HI, np.arange(n), _params(prob=prob, gamma_shape=0.0))
    rate = applied.mean()
    print('applied: rate %.4f for prob %.2f (5 se = %.4f)' % (rate, prob, 5 * np.sqrt(prob * (1 - prob) / n)))
    assert abs(rate - prob) <= 5.0 * np.sqrt(prob * (1.0 - prob) / n)
    assert np.all(host.scalars(SEED_LO, SEED_HI, np.arange(256), _params(prob=1.0))[1] == 1)
    assert np.all(host.scalars(SEED_LO, SEED_HI, np.arange(256), _params(prob=0.0))[1] == 0)


def test_draws_depend_on_their_keys_only():
    """An env's draws: the same alone and in a batch, the same whatever the image size beyond the grid index; different
    for another seed, draw index, env id or world seed."""
    p = _params(height=24, width=32, prob=1.0)
    g, applied, grid = host.draws(SEED_LO, SEED_HI, 7, p)
    gb, ab, _ = host.scalars(SEED_LO, SEED_HI, np.arange(16), p)
    assert _same(gb[7], g) and ab[7] == applied
    # a smaller image draws a prefix of the same sequence of grid values
    _, _, small = host.draws(SEED_LO, SEED_HI, 7, _params(height=8, width=12, prob=1.0))
    assert _same(small.ravel(), grid.ravel()[:small.size])
    g2, _, _ = host.draws(SEED_LO, SEED_HI, 7, _params(height=8, width=12, prob=1.0, sigma=0.0))
    assert _same(g2, g)
    for other in (dict(seed=1), dict(draw_index=1), dict(draw_index=(1 << 24) - 1)):
        q = dict(p); q.update(other)
        g3, _, grid3 = host.draws(SEED_LO, SEED_HI, 7, q)
        assert not np.array_equal(grid3, grid) and g3 != g
    for lo, hi, gid in ((SEED_LO, SEED_HI, 8), (SEED_LO + 1, SEED_HI, 7), (SEED_LO, SEED_HI + 1, 7)):
        g3, _, grid3 = host.draws(lo, hi, gid, p)
        assert not np.array_equal(grid3, grid) and g3 != g
    # the scalar blocks and the grid blocks do not meet
    assert host.SCALAR_BLOCK > (424 * 512) // 4


# ---- logr beyond 1
def test_logr_on_the_range_of_v():
    """The header extends logr's domain to what v = (1 + c x)^3 can be, [2^-72, 38]: against float64 over 2^22 points
    spread evenly in the exponent over [2^-72, 64), every float32 of [1 - 2^-10, 1 + 2^-10] and the powers of two.
    Contract: <= 1 ulp of the true value, or <= 2^-24 absolute on [1/2, 2] (where |log v| < 0.7)."""
    rng = np.random.default_rng(5)
    e = rng.uniform(-72.0, 6.0, 1 << 22)
    near = np.arange(F(1.0 - 2.0 ** -10).view(np.uint32), F(1.0 + 2.0 ** -10).view(np.uint32) + 1, dtype=np.uint32).view(F)
    x = np.concatenate([np.exp2(e).astype(F), near, np.exp2(np.arange(-72.0, 6.0)).astype(F), rng.uniform(0.5, 40.0, 1 << 20).astype(F)])
    got = logr(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    err = np.abs(got - want)
    ulps = err / np.maximum(_ulp32(want), 1e-300)
    mid = (x >= 0.5) & (x <= 2.0)
    ok = (ulps <= 1.0) | (mid & (err <= U))
    i = int(np.argmax(np.where(mid, 0.0, ulps)))
    print('logr on [2^-72, 64): max error %.3f ulp outside [1/2, 2] (at %r), max abs error %.3e inside'
          % (ulps[i], float(x[i]), err[mid].max()))
    assert np.all(ok), (x[~ok][:4], ulps[~ok][:4])
    assert logr(np.array([1.0], F))[0] == 0.0
    # the sign is right on both sides of 1
    assert np.all(got[x > 1.0] > 0.0) and np.all(got[x < 1.0] < 0.0)


# ---- ABI
def test_params_struct_has_the_c_layout():
    import subprocess
    import tempfile
    from robovat_amd import abi
    names = [n for n, _ in abi.rv_depth_noise_params._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rovat.h"\nint main(){printf("%zu", sizeof(rv_depth_noise_params));\n'
           + ''.join('printf(" %%zu", offsetof(rv_depth_noise_params, %s));\n' % n for n in names) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 't.c'), 'w') as f:
            f.write(src)
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(d, 't')], capture_output=True, text=True, check=True).stdout.split()]
    assert names == ['height', 'width', 'draw_index', 'seed', 'gamma_shape', 'prob', 'rescale_factor', 'sigma']
    assert out == [C.sizeof(abi.rv_depth_noise_params)] + [getattr(abi.rv_depth_noise_params, n).offset for n in names]


def test_symbol_and_params_builder():
    from robovat_amd import abi, configs, lib
    assert 'rv_depth_noise' in lib.SYMBOLS and 'rv_depth_noise' in abi.DEPTH_NOISE_API
    p = lib.depth_noise_params({'GAMMA_SHAPE': 2, 'PROB': 0.25, 'RESCALE_FACTOR': 2.0, 'SIGMA': 0.01, 'SEED': 9}, draw_index=5)
    assert (p.gamma_shape, p.prob, p.rescale_factor, p.seed, p.draw_index) == (2.0, 0.25, 2, 9, 5) and p.sigma == F(0.01)
    d = lib.depth_noise_params()
    assert (d.gamma_shape, d.prob, d.rescale_factor, d.seed) == (1000.0, 0.5, 4, 0) and d.sigma == F(0.005)
    assert lib.depth_noise_params({'RESCALE_FACTOR': 2.5}).rescale_factor == -1
    with pytest.raises(TypeError):
        lib.depth_noise_params({'GAMA_SHAPE': 2})
    with pytest.raises(TypeError):
        lib.depth_noise_params(sigmas=1)
    assert configs.grasp_env_config().OBSERVATION.DEPTH_NOISE is None
