"""The arithmetic of csrc/rv_dev_cem.h on the CPU, through its NumPy restatement tests/cem_host.py (the GPU tests pin the
kernels to that restatement bit for bit): the accuracy contract of logr, the moments of the keyed normals, the
independence of an env's candidates from batch and shard, and rv_cem_refit against a float64 version."""
import numpy as np
import pytest

import cem_host as host

F = np.float32
U = 2.0 ** -24      # the unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


# ---- logr
def test_logr_meets_its_contract_over_all_inputs():
    """Exhaustive over x = k 2^-24, k = 1 .. 2^24 (every u1 of the Box-Muller pair), against np.log in float64.  Contract of
    the header: <= 1 ulp of the true value (measured 0.83 at x = 0.702913), <= 2^-24 absolute for x >= 1/2 (measured
    3.94e-8), logr(1) = 0.  sincosr's contract is 2 ulp; this one is tighter."""
    x = (np.arange(1, (1 << 24) + 1, dtype=np.float64) * 2.0 ** -24).astype(F)
    got = host.logr(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    err = np.abs(got - want)
    assert got[-1] == 0.0 and not np.signbit(got[-1])
    assert np.all(got[:-1] < 0.0)
    nz = want != 0.0
    ulps = err[nz] / np.spacing(np.abs(want[nz]).astype(F)).astype(np.float64)
    i = int(np.argmax(ulps))
    near_one = err[x >= 0.5].max()
    print('logr: max error %.3f ulp of the true value at x = %r; max abs error %.3e for x >= 1/2' % (ulps[i], float(x[nz][i]), near_one))
    assert ulps[i] <= 1.0, 'logr: %.3f ulp at x = %r (contract 1 ulp)' % (ulps[i], float(x[nz][i]))
    assert near_one <= 2.0 ** -24


# ---- the normals
@pytest.fixture(scope='module')
def normals():
    """2^20 normals from fixed keys: world seed 0, env ids 0 .. 3, plan_index 0, iteration 0, policy seed 0, the 1024
    candidates x 64 blocks of each env.  [4, 1024, 64, 4]; the last axis is (pair 0: cos, sin; pair 1: cos, sin)."""
    j, q = np.arange(1024)[:, None], np.arange(64)[None, :]
    z = np.stack([host.normals(0, gid, 0, 0, 0, j, q) for gid in range(4)])
    assert z.size == 1 << 20 and z.dtype == F
    z.setflags(write=False)
    return z


def test_normals_mean_and_variance(normals):
    z = normals.astype(np.float64).ravel()
    n = z.size
    print('normals: mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)' % (z.mean(), 5 / np.sqrt(n), z.var() - 1, 5 * np.sqrt(2.0 / n)))
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


def test_normals_kolmogorov_smirnov(normals):
    from scipy import stats
    z = np.sort(normals.astype(np.float64).ravel())
    n = z.size
    cdf = stats.norm.cdf(z)
    d = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(0, n) / n).max())
    print('normals: KS statistic %.3e (bound %.3e)' % (d, 1.95 / np.sqrt(n)))
    assert d <= 1.95 / np.sqrt(n)


def test_normals_are_bounded_and_finite(normals):
    assert np.isfinite(normals).all()
    assert np.abs(normals).max() <= 5.78
    # the bound of the header: r <= sqrt(-2 log 2^-24) = 5.7681 for the smallest u1 there is
    r = np.sqrt(F(-2.0) * host.logr(np.array([2.0 ** -24], F)))[0]
    assert 5.76 < r <= 5.77
    z0, z1 = host.normal_pair(np.array([0, 0xffffffff], np.uint64), np.array([0, 0], np.uint64))
    # u1 = 2^-24 and u1 = 1, angle 0: (r, 0) and (0, 0) -- the latter zeros of either sign: r = sqrt(-2 * 0) = -0
    assert z0[0] == r and z0[1] == 0.0 and np.all(z1 == 0.0)


def test_members_of_a_pair_are_uncorrelated(normals):
    z = normals.astype(np.float64).reshape(-1, 2)
    rho = np.corrcoef(z[:, 0], z[:, 1])[0, 1]
    n = normals.size
    print('normals: correlation within a pair %.3e (bound %.3e)' % (rho, 5 / np.sqrt(n)))
    assert abs(rho) <= 5.0 / np.sqrt(n)


# ---- keys
def _dist(n, d, seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(-0.5, 0.5, (n, d)).astype(F), rng.uniform(0.1, 0.6, (n, d)).astype(F)


def test_an_envs_candidates_do_not_depend_on_batch_sample_count_or_shard():
    mean, std = _dist(7, 24)
    kw = dict(world_seed=9, plan_index=3, iteration=1, seed=5, keep_mean=False)
    full = host.cem_sample(mean, std, 64, **kw)
    assert _same(host.cem_sample(mean[:1], std[:1], 64, **kw), full[:1])                       # N = 1 and N = 7
    assert _same(host.cem_sample(mean, std, 4, **kw), full[:, :4])                             # S = 4 and S = 64
    assert _same(host.cem_sample(mean[2:5], std[2:5], 64, env_id_offset=2, **kw), full[2:5])   # a shard at offset 2
    assert _same(host.cem_sample(mean[:, :8], std[:, :8], 64, **kw), full[:, :, :8])           # H = 2 and H = 6 (A = 4)
    shifted = host.cem_sample(mean, std, 64, env_id_offset=1, **kw)
    same_dist = host.cem_sample(np.repeat(mean[:1], 2, 0), np.repeat(std[:1], 2, 0), 8, **kw)
    assert not _same(same_dist[0], same_dist[1])                                               # env id
    assert not _same(shifted[0], full[0])
    for other in (dict(kw, seed=6), dict(kw, plan_index=4), dict(kw, iteration=2), dict(kw, world_seed=10), dict(kw, world_seed=9 + (1 << 32))):
        assert not _same(host.cem_sample(mean[:1], std[:1], 8, **other), full[:1, :8]), other
    # distinct counter words for distinct (iteration, j, q): no two candidates of an env share a block
    z = host.normals(9, 0, 3, 1, 5, np.arange(1024)[:, None], np.arange(128)[None, :]).reshape(-1, 4)
    assert len(np.unique(_bits(z), axis=0)) == len(z)


def test_keep_mean_std_zero_and_the_clamp():
    mean, std = _dist(2, 16, seed=1)
    mean[0, :4] = [1.5, -1.5, 1.0, -1.0]
    kept = host.cem_sample(mean, std, 5, keep_mean=True)
    drawn = host.cem_sample(mean, std, 5, keep_mean=False)
    assert _same(kept[:, 0], np.clip(mean, -1, 1)) and _same(kept[:, 1:], drawn[:, 1:]) and not _same(kept[:, 0], drawn[:, 0])
    flat = host.cem_sample(mean, np.zeros_like(std), 5, keep_mean=False)                     # std = 0: every candidate is clamp(mean)
    assert _same(flat, np.broadcast_to(np.clip(mean, -1, 1)[:, None], flat.shape).copy())
    for m in (1.0, -1.0):                                                                     # mean on the bound, std 1
        x = host.cem_sample(np.full((1, 64), m, F), np.ones((1, 64), F), 256, keep_mean=False)
        at = np.mean(x == F(m))
        print('mean %+.0f, std 1: %.3f of the draws on the bound' % (m, at))
        assert np.abs(x).max() <= 1.0 and 0.4 < at < 0.6 and np.mean(x == F(-m)) < 0.05


# ---- the ranking order
def test_ranking_order_edge_cases():
    nan, inf = np.nan, np.inf
    r = np.array([[0.0, nan, -inf, 3.0, -0.0, inf, 3.0, -nan, -1.0, 0.0]], F)
    order = host.cem_rank(r)[0].tolist()
    assert order == [5, 3, 6, 0, 4, 9, 8, 2, 1, 7]      # +inf, the 3s by index, +-0 as equals by index, -1, -inf, the NaNs by index
    assert host.cem_rank(np.full((2, 9), 2.5, F)).tolist() == [list(range(9))] * 2      # all equal: 0 .. S-1
    assert host.cem_rank(np.array([[nan]], F)).tolist() == [[0]]      # S = 1
    key = host.cem_key(np.array([-inf, nan, -nan], F))
    assert key[0] == 0xff800000 and key[1] == key[2] == 0xffffffff
    # the key reverses the order of the numbers exactly
    rng = np.random.RandomState(0)
    v = np.sort(np.concatenate([rng.standard_normal(1000).astype(F) * F(100), [F(inf), F(-inf), F(0), F(1e-45), F(-1e-45)]]).astype(F))
    k = host.cem_key(v).astype(np.int64)
    assert np.all((np.diff(k) < 0) == (np.diff(v) > 0)) and np.all((np.diff(k) == 0) == (np.diff(v) == 0))


def _refit64(x, returns, e):
    """the float64 version: a stable argsort of -returns (NaNs last), mean and std(ddof=0) of the elites"""
    order = np.argsort(-returns.astype(np.float64), axis=1, kind='stable')[:, :e]
    xe = np.take_along_axis(x.astype(np.float64), order[:, :, None], axis=1)
    return order.astype(np.int32), xe.mean(axis=1), xe.var(axis=1, ddof=0)


@pytest.mark.parametrize('s,e', [(1, 1), (5, 1), (5, 5), (64, 8), (200, 25), (1024, 128), (1024, 1024)])
def test_refit_against_float64(s, e):
    """Bounds, from E and |x| <= 1 with u = 2^-24.  The sum of E terms in sequence is off by at most (E - 1) u E (every
    partial sum is at most E), so the mean by (E - 1) u plus its own rounding u: (E + 1) u covers it.  A deviation
    x - m is at most 2 and carries u relative, its square 3 u relative of at most 4: 12 u per term; the sequential sum of
    E such terms adds (E - 1) u 4 E, the division by E brings that to 4 (E - 1) u and rounds once more (4 u); the error
    dm of the mean adds dm^2 exactly (sum (x - m) = 0): (4 E + 12) u + ((E + 1) u)^2."""
    rng = np.random.RandomState(s * 7 + e)
    n, d = 3, 12
    x = rng.uniform(-1, 1, (n, s, d)).astype(F)
    x[0, :, 0] = 1.0; x[0, :, 1] = -1.0; x[0, :, 2] = F(0.3)      # constant columns: variance 0 (2) only up to the bound
    returns = rng.standard_normal((n, s)).astype(F)
    returns[1, : s // 2] = returns[1, 0]      # ties
    mean0, std0 = _dist(n, d, seed=3)
    mean, std, elite = host.cem_refit(x, returns, mean0, std0, e)
    order, m64, v64 = _refit64(x, returns, e)
    assert elite.dtype == np.int32 and np.array_equal(elite, order)
    m, v = host.elite_moments(np.take_along_axis(x, elite[:, :, None].astype(np.int64), axis=1))
    b_mean = (e + 1) * U
    b_var = (4 * e + 12) * U + b_mean ** 2
    print('S=%d E=%d: mean error %.3e (bound %.3e), variance error %.3e (bound %.3e)' %
          (s, e, np.abs(m - m64).max(), b_mean, np.abs(v - v64).max(), b_var))
    assert np.abs(m.astype(np.float64) - m64).max() <= b_mean
    assert np.abs(v.astype(np.float64) - v64).max() <= b_var
    # alpha = 0, no floor: the new distribution IS the elites' (mean bit for bit; std^2 within the root's own rounding,
    # 2 u relative of at most 4)
    assert _same(mean, m) and _same(std, np.sqrt(v))
    assert np.abs(std.astype(np.float64) ** 2 - v64).max() <= b_var + 8 * U
    assert v[0, 0] == 0.0 and v[0, 1] == 0.0      # exactly representable constants: no spurious spread


def test_refit_ranking_with_special_returns():
    rng = np.random.RandomState(5)
    x = rng.uniform(-1, 1, (1, 10, 8)).astype(F)
    r = np.array([[0.0, np.nan, -np.inf, 3.0, -0.0, np.inf, 3.0, np.nan, -1.0, 0.0]], F)
    mean0, std0 = _dist(1, 8)
    for e, want in ((1, [5]), (3, [5, 3, 6]), (10, [5, 3, 6, 0, 4, 9, 8, 2, 1, 7])):
        mean, std, elite = host.cem_refit(x, r, mean0, std0, e)
        assert elite[0].tolist() == want
        assert np.allclose(mean[0], x[0, want].astype(np.float64).mean(axis=0), atol=(e + 1) * U, rtol=0)
    mean, std, elite = host.cem_refit(x[:, :1], r[:, 1:2], mean0, std0, 1)      # S = 1, its return a NaN
    assert elite.tolist() == [[0]] and _same(mean, x[:, 0]) and _same(std, np.zeros((1, 8), F))


def test_refit_smoothing_and_floor():
    rng = np.random.RandomState(6)
    x = rng.uniform(-1, 1, (2, 16, 8)).astype(F)
    x[:, :, 0] = F(0.25)      # no spread in column 0
    r = rng.standard_normal((2, 16)).astype(F)
    mean0, std0 = _dist(2, 8, seed=7)
    m0, s0, el = host.cem_refit(x, r, mean0, std0, 4, alpha=0.0, min_std=0.0)
    m5, s5, el5 = host.cem_refit(x, r, mean0, std0, 4, alpha=0.5, min_std=0.0)
    assert np.array_equal(el, el5)
    assert _same(m5, F(0.5) * mean0 + F(0.5) * m0) and _same(s5, F(0.5) * std0 + F(0.5) * s0)
    assert np.all(s0[:, 0] == 0.0) and np.all(m0[:, 0] == F(0.25))
    mf, sf, _ = host.cem_refit(x, r, mean0, std0, 4, alpha=0.0, min_std=0.3)
    assert _same(mf, m0) and _same(sf, np.maximum(s0, F(0.3))) and np.all(sf[:, 0] == F(0.3)) and np.any(sf > F(0.3))
    m9, s9, _ = host.cem_refit(x, r, mean0, std0, 4, alpha=0.9, min_std=0.0)
    oma = F(1.0) - F(0.9)      # (1 - alpha in float32, once)
    assert _same(m9, F(0.9) * mean0 + oma * m0) and _same(s9, F(0.9) * std0 + oma * s0)
