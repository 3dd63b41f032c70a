"""NumPy restatement of csrc/rv_dev_depth_noise.h (rv_depth_noise), for the tests: float32, operation for operation, every
product and sum rounded on its own.  Two parts: ``draws`` (the keyed per-image scalars and the noise grid of one env) and
``apply`` (the gamma multiplier and the bicubic upsampling on a batch of images).  logr, normal_pair and the Philox block
come from tests/cem_host.py / tests/antipodal_host.py."""
import numpy as np

from antipodal_host import philox
from cem_host import logr, normal_pair

F = np.float32
RV_STREAM_DEPTH_NOISE = 9
SCALAR_BLOCK = 0x80000000
TWO_M24 = F(5.9604644775390625e-8)
THIRD = F(0.333333343)
FIELDS = ('height', 'width', 'draw_index', 'seed', 'gamma_shape', 'prob', 'rescale_factor', 'sigma')


def fields(params):
    """params (a mapping or an rv_depth_noise_params) -> dict of plain numbers"""
    get = (lambda k: params[k]) if isinstance(params, dict) else (lambda k: getattr(params, k))
    p = {k: get(k) for k in FIELDS}
    assert 0 <= p['draw_index'] < (1 << 24) and 1 <= p['rescale_factor'] <= 8
    assert p['height'] % p['rescale_factor'] == 0 and p['width'] % p['rescale_factor'] == 0
    return p


def block(seed_lo, seed_hi, gid, p, c0):
    """dn_block: the Philox words of counter c0 (an array) -> four uint64 arrays holding 32-bit words"""
    c0 = np.asarray(c0, np.uint64)
    c3 = (RV_STREAM_DEPTH_NOISE << 24) | int(p['draw_index'])
    return philox(c0, np.full_like(c0, int(p['seed']) & 0xFFFFFFFF), np.full_like(c0, gid), np.full_like(c0, c3),
                  seed_lo, seed_hi)


def gamma_attempt(o, k):
    """one Marsaglia-Tsang attempt from the words o = (o0, o1, o2) (arrays) -> (accepted, g)"""
    k = F(k)
    d = k - THIRD
    c = F(1.0) / np.sqrt(F(9.0) * d)
    x, _ = normal_pair(o[0], o[1])
    t1 = F(1.0) + c * x
    v = (t1 * t1) * t1
    u = ((np.asarray(o[2], np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(F) * TWO_M24
    x2 = x * x
    x4 = x2 * x2
    pos = v > F(0.0)
    vs = np.where(pos, v, F(1.0))      # (logr is not evaluated where v <= 0)
    squeeze = u < F(1.0) - F(0.0331) * x4
    full = logr(u) < F(0.5) * x2 + d * ((F(1.0) - vs) + logr(vs))
    return pos & (squeeze | full), ((d * v) / k).astype(F)


def scalars(seed_lo, seed_hi, gid, p):
    """dn_scalars for the envs gid (an array) -> (g float32, applied uint8, attempts used; 4 = the fallback g = 1)"""
    gid = np.atleast_1d(np.asarray(gid, np.uint64))
    o = block(seed_lo, seed_hi, gid, p, np.full_like(gid, SCALAR_BLOCK))
    applied = ((o[3] >> np.uint64(8)).astype(F) * TWO_M24 < F(p['prob'])).astype(np.uint8)
    g = np.ones(gid.shape, F)
    used = np.zeros(gid.shape, np.int32)
    if F(p['gamma_shape']) != F(0.0):
        used[:] = 4
        open_ = np.ones(gid.shape, bool)
        for t in range(4):
            if t > 0:
                o = block(seed_lo, seed_hi, gid, p, np.full_like(gid, SCALAR_BLOCK | t))
            ok, gt = gamma_attempt(o, p['gamma_shape'])
            take = open_ & ok
            g[take] = gt[take]
            used[take] = t
            open_ &= ~ok
    return g, applied, used


def grid_normals(seed_lo, seed_hi, gid, p, count):
    """the first `count` standard normals of env gid's noise grid, float32"""
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    o = block(seed_lo, seed_hi, np.full_like(q, gid), p, q)
    z0, z1 = normal_pair(o[0], o[1])
    z2, z3 = normal_pair(o[2], o[3])
    return np.stack([z0, z1, z2, z3], axis=-1).astype(F).reshape(-1)[:count]


def draws(seed_lo, seed_hi, gid, params):
    """k_depth_noise_draw for the env with global id gid -> (g float32, applied 0 / 1, grid float32 [H / R, W / R]; zeros
    where the kernel writes nothing: the env is not applied, or sigma is 0)"""
    p = fields(params)
    g, applied, _ = scalars(seed_lo, seed_hi, gid, p)
    h, w = p['height'] // p['rescale_factor'], p['width'] // p['rescale_factor']
    grid = np.zeros((h, w), F)
    if applied[0] and F(p['sigma']) > F(0.0):
        grid = (F(p['sigma']) * grid_normals(seed_lo, seed_hi, gid, p, h * w)).astype(F).reshape(h, w)
    return F(g[0]), int(applied[0]), grid


def keys(t):
    """dn_keys: Keys' cubic, a = -0.5, on float32 arrays"""
    t = np.abs(np.asarray(t, F))
    inner = ((F(1.5) * t - F(2.5)) * t) * t + F(1.0)
    outer = (((t - F(5.0)) * t + F(8.0)) * t - F(4.0)) * F(-0.5)
    return np.where(t < F(1.0), inner, np.where(t < F(2.0), outer, F(0.0))).astype(F)


def taps(n_out, R, n_in):
    """dn_taps for every output index of an axis -> (lo int [n_out], nt int [n_out], w float32 [n_out, 4])"""
    xx = np.arange(n_out)
    center = (xx.astype(F) + F(0.5)) / F(R)
    lo = np.maximum(((center - F(2.0)) + F(0.5)).astype(np.int32), 0)      # (astype truncates towards zero, as the C cast)
    hi = np.minimum(((center + F(2.0)) + F(0.5)).astype(np.int32), n_in)
    nt = np.minimum(hi - lo, 4)
    w = np.zeros((n_out, 4), F)
    ww = np.zeros(n_out, F)
    for k in range(4):
        on = k < nt
        wk = keys(((lo + k).astype(F) - center) + F(0.5))
        w[:, k] = np.where(on, wk, F(0.0))
        ww = np.where(on, ww + w[:, k], ww).astype(F)
    for k in range(4):
        on = k < nt
        w[:, k] = np.where(on, w[:, k] / np.where(on, ww, F(1.0)), F(0.0))
    return lo, nt, w


def resample(a, R, axis):
    """one pass of the resize along `axis` of float32 [..., rows, cols] (-1: horizontal, -2: vertical)"""
    a = np.moveaxis(np.asarray(a, F), axis, -1)
    n_in = a.shape[-1]
    lo, nt, w = taps(n_in * R, R, n_in)
    out = np.zeros(a.shape[:-1] + (n_in * R,), F)
    for k in range(4):
        on = k < nt
        v = a[..., np.minimum(lo + k, n_in - 1)]
        out = np.where(on, out + v * w[:, k], out).astype(F)
    return np.moveaxis(out, -1, axis)


def upsample(grid, R):
    """up(grid): float32 [..., h, w] -> [..., h R, w R]; the horizontal pass first, then the vertical"""
    return resample(resample(grid, R, -1), R, -2)


def apply(depth, g, applied, grid, R):
    """k_depth_noise_apply: depth [N, H, W], g [N], applied [N], grid [N, H / R, W / R] -> float32 [N, H, W]"""
    depth = np.ascontiguousarray(depth, F)
    g = np.asarray(g, F).reshape(-1, 1, 1)
    on = np.asarray(applied).reshape(-1, 1, 1) != 0
    o = (depth * g).astype(F)
    up = upsample(np.asarray(grid, F), int(R))
    return np.where(on & (o > F(0.0)), o + up, o).astype(F)
