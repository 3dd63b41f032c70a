"""NumPy restatement of csrc/rv_dev_cem.h (rv_cem_sample / rv_cem_refit), for the tests: float32, operation for
operation, every product and sum rounded on its own.  Also restated here, because the normals need them: sincosr of
rv_dev_math.h (with its two fused multiply-adds next to a zero, emulated exactly) and the Philox block of
tests/antipodal_host.py."""
import numpy as np

from antipodal_host import philox

F = np.float32
U32 = np.uint32
RV_STREAM_CEM = 8
RV_CEM_MAX_SAMPLES, RV_CEM_MAX_DIM = 1024, 512
TWO_PI = F(6.283185307179586)
TWO_M24 = F(5.9604644775390625e-8)


def logr(x):
    """logr: x float32 in (0, 1], normal"""
    x = np.ascontiguousarray(x, F)
    ix = x.view(U32) + U32(0x3f800000 - 0x3f3504f3)
    k = (ix >> U32(23)).astype(np.int32) - np.int32(127)
    ix = (ix & U32(0x007fffff)) + U32(0x3f3504f3)
    f = ix.view(F) - F(1.0)
    s = f / (F(2.0) + f)
    z = s * s
    w = z * z
    t1 = w * (F(0.40000972152) + w * F(0.24279078841))
    t2 = z * (F(0.66666662693) + w * F(0.28498786688))
    R = t2 + t1
    hfsq = (F(0.5) * f) * f
    dk = k.astype(F)
    return (((s * (hfsq + R) + dk * F(9.0580006145e-6)) - hfsq) + f) + dk * F(6.9313812256e-1)


def fma(a, b, c):
    """rv_fma on float32 arrays: a * b + c with one rounding.  The product of two float32 is exact in float64; the sum is
    rounded to odd in float64 (TwoSum gives its error), so that the final rounding to float32 is the only one that counts."""
    p = np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64)
    c = np.asarray(c, F).astype(np.float64)
    hi = p + c
    bb = hi - p
    err = (p - (hi - bb)) + (c - bb)
    even = (hi.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even
    toward = np.where((err > 0), np.inf, -np.inf)
    return np.where(fix, np.nextafter(hi, toward), hi).astype(F)


def sincosr(x):
    """sincosr of rv_dev_math.h -> (sin, cos)"""
    x = np.ascontiguousarray(x, F)
    k = np.rint(x * F(0.636619772367581343)).astype(F)
    t = (x - k * F(1.5703125)) - k * F(4.837512969970703125e-4)
    r = t - k * F(7.54978995489188216e-8)
    near = np.abs(r) < F(1.52587890625e-5)
    r = np.where(near, fma(-k, np.full_like(k, F(-1.7151245100058819e-15)), fma(-k, np.full_like(k, F(7.54978995489188216e-8)), t)), r)
    z = r * r
    sp = r + r * z * (F(-1.6666654611e-1) + z * (F(8.3321608736e-3) + z * F(-1.9515295891e-4)))
    cp = F(1.0) - F(0.5) * z + z * z * (F(4.166664568298827e-2) + z * (F(-1.388731625493765e-3) + z * F(2.443315711809948e-5)))
    q = k.astype(np.int32) & 3
    odd = (q & 1) == 1
    ss, cc = np.where(odd, cp, sp), np.where(odd, sp, cp)
    cc = np.where((q == 1) | (q == 2), -cc, cc)
    ss = np.where(q >= 2, -ss, ss)
    return ss.astype(F), cc.astype(F)


def normal_pair(a, b):
    """normal_pair: two uint32 Philox words (arrays) -> (z0, z1)"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(F) * TWO_M24
    u2 = (b >> np.uint64(8)).astype(F) * TWO_M24
    r = np.sqrt(F(-2.0) * logr(u1))
    sn, cs = sincosr(TWO_PI * u2)
    return r * cs, r * sn


def normals(world_seed, gid, plan_index, iteration, seed, j, q):
    """cem_normals: the four normals of every (j, q) pair (broadcast arrays) -> float32 [..., 4]"""
    j, q = np.broadcast_arrays(np.asarray(j, np.uint64), np.asarray(q, np.uint64))
    assert 0 <= iteration < (1 << 15) and 0 <= plan_index < (1 << 24) and j.max() < 1024 and q.max() < 128
    c0 = (np.uint64(iteration) << np.uint64(17)) | (j << np.uint64(7)) | q
    c3 = (RV_STREAM_CEM << 24) | plan_index
    o = philox(c0, np.full_like(c0, seed & 0xFFFFFFFF), np.full_like(c0, gid), np.full_like(c0, c3),
               world_seed & 0xFFFFFFFF, world_seed >> 32)
    z0, z1 = normal_pair(o[0], o[1])
    z2, z3 = normal_pair(o[2], o[3])
    return np.stack([z0, z1, z2, z3], axis=-1).astype(F)


def fclampr(x, lo, hi):
    return np.where(x < lo, F(lo), np.where(x > hi, F(hi), x)).astype(F)


def cem_sample(mean, std, s, world_seed=0, env_id_offset=0, plan_index=0, iteration=0, seed=0, keep_mean=True):
    """k_cem_sample: mean, std [N, D] -> float32 [N, s, D]"""
    mean, std = np.ascontiguousarray(mean, F), np.ascontiguousarray(std, F)
    N, D = mean.shape
    assert D % 4 == 0 and D <= RV_CEM_MAX_DIM and 1 <= s <= RV_CEM_MAX_SAMPLES
    out = np.empty((N, s, D), F)
    j, q = np.arange(s)[:, None], np.arange(D // 4)[None, :]
    for n in range(N):
        z = normals(world_seed, env_id_offset + n, plan_index, iteration, seed, j, q).reshape(s, D)
        out[n] = fclampr(mean[n][None] + std[n][None] * z, -1.0, 1.0)
        if keep_mean:
            out[n, 0] = fclampr(mean[n], -1.0, 1.0)
    return out


def cem_key(r):
    """cem_key: float32 returns -> the uint32 sort keys"""
    r = np.ascontiguousarray(r, F)
    b = r.view(U32).copy()
    b[b == U32(0x80000000)] = U32(0)
    key = ~(b ^ np.where((b >> U32(31)) != 0, U32(0xffffffff), U32(0x80000000)))
    return np.where(np.isnan(r), U32(0xffffffff), key).astype(U32)


def cem_rank(returns):
    """the order of k_cem_refit (a): returns [N, S] -> indices int32 [N, S], best first"""
    key = cem_key(returns).astype(np.uint64)
    word = (key << np.uint64(32)) | np.arange(key.shape[-1], dtype=np.uint64)
    return (np.sort(word, axis=-1) & np.uint64(0xffffffff)).astype(np.int32)


def elite_moments(xe):
    """k_cem_refit (c) up to the root: xe [N, E, D], the elites in rank order -> (m, v) float32 [N, D]"""
    xe = np.ascontiguousarray(xe, F)
    N, E, D = xe.shape
    total = np.zeros((N, D), F)
    for k in range(E):
        total = total + xe[:, k]
    m = total / F(E)
    v = np.zeros((N, D), F)
    for k in range(E):
        dl = xe[:, k] - m
        v = v + dl * dl
    return m, v / F(E)


def cem_refit(actions, returns, mean, std, n_elites, alpha=0.0, min_std=0.0):
    """k_cem_refit: actions [N, S, D], returns [N, S], mean / std [N, D] -> (mean', std', elite int32 [N, E])"""
    x = np.ascontiguousarray(actions, F)
    mean, std = np.ascontiguousarray(mean, F), np.ascontiguousarray(std, F)
    N, S, D = x.shape
    E = int(n_elites)
    assert 1 <= E <= S
    elite = cem_rank(np.ascontiguousarray(returns, F).reshape(N, S))[:, :E]
    xe = np.take_along_axis(x, elite[:, :, None].astype(np.int64), axis=1)      # [N, E, D], rank order
    m, v = elite_moments(xe)
    sd = np.sqrt(v)
    alpha, oma = F(alpha), F(1.0) - F(alpha)
    new_mean = alpha * mean + oma * m
    st = alpha * std + oma * sd
    new_std = np.where(st > F(min_std), st, F(min_std)).astype(F)      # (fmaxr: a > b ? a : b)
    return new_mean.astype(F), new_std, elite
