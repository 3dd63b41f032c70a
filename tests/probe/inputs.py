"""The inputs of the math-primitive tests: ONE deterministic generator shared by tests/test_math_primitives.py (CPU)
and tests/test_gpu_math_primitives.py (device).  No input is a NaN and -- checked by the CPU test -- no output of
the float functions is one either, so bit parity never has to compare NaN payloads.

``cases()`` maps the name of every probe function to its input arrays (and ``k`` for the rng streams).
"""
import functools
import math

import numpy as np

F = np.float32
FLT_MIN = F(2.0 ** -126)
FLT_MAX = np.finfo(F).max
DEN_MIN = F(2.0 ** -149)
DEN_MAX = np.nextafter(FLT_MIN, F(0))
SINCOS_MAX = 1.0e4              # the documented domain of sincosr (rv_dev_math.h)
RANDINT_N = (1, 2, 3, 7, 64, 2 ** 31 - 1)


def _ulps(x, d):
    """x moved by d float ulps (d integer, array or scalar), through the ordered integer view of the bits."""
    x = np.asarray(x, F)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i)          # sign-magnitude -> ordered
    i = i + d
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(F)


def _cat(*parts):
    return np.concatenate([np.asarray(p, F).ravel() for p in parts])


@functools.lru_cache(maxsize=None)
def scalars():
    """Every power of two in range, +-0, the smallest and largest denormal, FLT_MIN, FLT_MAX, 1 +- 1 ulp, small
    integers and half-integers (ties of rint), and 2^20 points log-uniform over ALL finite magnitudes (uniform over
    the bit patterns 1 .. FLT_MAX, denormals included) with random signs."""
    rng = np.random.default_rng(20240)
    pow2 = np.array([2.0 ** e for e in range(-149, 128)], np.float64).astype(F)
    halves = np.arange(-64, 65, dtype=np.float64) + 0.5
    big = [2.0 ** 22 + 0.5, 2.0 ** 23 - 0.5, 2.0 ** 23 + 1, 2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 31, 2.0 ** 31 - 128]
    special = _cat([0.0, -0.0, DEN_MIN, DEN_MAX, FLT_MIN, FLT_MAX, 1.0], _ulps(F(1), np.array([-1, 1])),
                   _ulps(FLT_MIN, np.array([-1, 1])), np.arange(-64, 65), halves, _ulps(halves.astype(F), 1),
                   _ulps(halves.astype(F), -1), big)
    bits = rng.integers(1, 0x7F7FFFFF, size=1 << 20, endpoint=True, dtype=np.int64).astype(np.uint32)
    sweep = bits.view(F) * np.where(rng.integers(0, 2, bits.size) == 1, F(-1), F(1))
    pos = _cat(pow2, special)
    return _cat(pos, -pos, sweep)


def _perm(x, seed):
    return x[np.random.default_rng(seed).permutation(x.size)]


@functools.lru_cache(maxsize=None)
def division_pairs():
    """(a, b) for a / b: the scalars against a permutation of themselves (0 / 0 replaced), pairs whose quotient is a
    denormal, and pairs whose quotient is an exact tie between two floats.  Division cannot produce an exact tie in
    the normal range (an odd 25-bit quotient times an odd divisor is odd); in the denormal range it can, when the bits
    shifted out are 100...0 -- there the quotient is exact in double and a tie for float."""
    rng = np.random.default_rng(20241)
    a = scalars()
    b = _perm(a, 1)
    b = np.where((a == 0) & (b == 0), F(1), b)
    # denormal quotients: a in [2^-126, 2^-100), b in [1, 2^40)
    n = 1 << 16
    a2 = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-126, -100, n)).astype(F)
    b2 = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(0, 40, n)).astype(F)
    # exact ties: a = M 2^-149 with the low t bits of M equal to 1 0...0, b = 2^t or 3 2^t (then M is a multiple of 3)
    t = rng.integers(1, 24, n)
    m = rng.integers(1 << 20, 1 << 22, n)
    m = ((m >> t) << t) | (1 << (t - 1))
    three = rng.integers(0, 2, n) == 1
    a3 = (np.where(three, 3 * m, m).astype(np.float64) * 2.0 ** -149).astype(F)       # 3 m < 2^24: exact
    b3 = (np.where(three, 3.0, 1.0) * 2.0 ** t).astype(F)
    sign = np.where(rng.integers(0, 2, n) == 1, F(-1), F(1))
    q = a3.astype(np.float64) / b3.astype(np.float64) / 2.0 ** -149
    assert (q - np.floor(q) == 0.5).all()                                              # ties indeed
    return _cat(a, a2, a3 * sign), _cat(b, b2, b3)


@functools.lru_cache(maxsize=None)
def sqrt_inputs():
    """x >= 0 and -0 (a negative x gives a NaN, whose sign is not the same on every machine).  A square root is never
    a denormal or a tie; the denormal INPUTS are here."""
    s = scalars()
    return _cat(s[s >= 0], [-0.0])


@functools.lru_cache(maxsize=None)
def clamp_pairs():
    """(x, b), b > 0: x over the scalars and +-inf, b over a permutation of their magnitudes (denormals included);
    then x = +-b, +-b one ulp in and out, and +-0 against every b."""
    s = scalars()
    b = np.abs(_perm(s, 2)); b = np.where(b == 0, DEN_MIN, b)
    x = s
    edge_b = b[:4096]
    xs = [x, [np.inf, -np.inf], edge_b, -edge_b, _ulps(edge_b, 1), _ulps(edge_b, -1), -_ulps(edge_b, 1), -_ulps(edge_b, -1),
          np.zeros(4096, F), -np.zeros(4096, F)]
    bs = [b, [DEN_MIN, FLT_MAX]] + [edge_b] * 8
    return _cat(*xs), _cat(*bs)


@functools.lru_cache(maxsize=None)
def fma_triples():
    """(a, b, c): permutations of the scalars, then c = -round(a b) for moderate a, b: the fused result is the exact
    rounding error of the product (zero for an unfused multiply-add)."""
    s = scalars()
    a, b, c = s, _perm(s, 3), _perm(s, 4)
    rng = np.random.default_rng(20242)
    a2 = rng.uniform(-4, 4, 1 << 16).astype(F); b2 = rng.uniform(-4, 4, 1 << 16).astype(F)
    c2 = -(a2 * b2)
    return _cat(a, a2), _cat(b, b2), _cat(c, c2)


@functools.lru_cache(maxsize=None)
def sincos_inputs():
    """|x| <= 26 and |x| <= 1e4 uniform (2^20 points each); (k + 1/2) pi/2 -- the ties of rint(x 2/pi), where the
    quadrant switches -- and k pi/2, k = -64..64, each -2..2 ulp around its float; +-0 and denormals.  Nothing beyond
    the documented domain 1e4."""
    rng = np.random.default_rng(20243)
    k = np.arange(-64, 65, dtype=np.float64)
    d = np.arange(-2, 3)
    ties = _ulps(((k + 0.5) * (math.pi / 2)).astype(F)[:, None], d[None, :])
    mults = _ulps((k * (math.pi / 2)).astype(F)[:, None], d[None, :])
    x = _cat(rng.uniform(-26, 26, 1 << 20), rng.uniform(-SINCOS_MAX, SINCOS_MAX, 1 << 20), ties, mults,
             [0.0, -0.0, DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX, FLT_MIN, -FLT_MIN, 26.0, -26.0, SINCOS_MAX, -SINCOS_MAX])
    assert (np.abs(x) <= F(SINCOS_MAX)).all()
    return x


ATAN_T0, ATAN_T1 = F(0.4142135623730950), F(2.414213562373095)      # the branch thresholds of atan_pos


@functools.lru_cache(maxsize=None)
def atan_pos_inputs():
    """x >= 0: the non-negative scalars, +inf, both thresholds -2..2 ulp, 2^20 points log-uniform in [1e-6, 1e6]."""
    rng = np.random.default_rng(20244)
    s = scalars()
    d = np.arange(-2, 3)
    return _cat(s[s >= 0], [np.inf], _ulps(ATAN_T0, d), _ulps(ATAN_T1, d), 10.0 ** rng.uniform(-6, 6, 1 << 20))


@functools.lru_cache(maxsize=None)
def atan2_inputs():
    """(y, x).  2^20 points on circles of radius 10^u, u uniform in [-6, 6]; ratios at the two thresholds of atan_pos
    -2..2 ulp in all four quadrants; the axes with both signed zeros; denormal / huge / infinite components."""
    rng = np.random.default_rng(20245)
    n = 1 << 20
    th = rng.uniform(-math.pi, math.pi, n); r = 10.0 ** rng.uniform(-6, 6, n)
    ys, xs = [r * np.sin(th)], [r * np.cos(th)]
    t = _cat(_ulps(ATAN_T0, np.arange(-2, 3)), _ulps(ATAN_T1, np.arange(-2, 3)))
    for sy in (1, -1):
        for sx in (1, -1):
            ys.append(sy * t); xs.append(np.full(t.size, sx, F))
            ys.append(sy * t * F(3)); xs.append(np.full(t.size, 3 * sx, F))
    z = [0.0, -0.0]
    one = [1.0, -1.0]
    den = [DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX]
    inf = [np.inf, -np.inf]
    pairs = [(a, b) for a in z for b in z] + [(a, b) for a in z for b in one] + [(a, b) for a in one for b in z]
    pairs += [(a, b) for a in den for b in one] + [(a, b) for a in one for b in den]
    pairs += [(1e38, 1e-38), (1e-38, 1e38), (-1e38, 1e-38), (1e-38, -1e38), (1e38, -1e-38), (-1e-38, 1e38)]
    pairs += [(a, b) for a in inf for b in one + [3.0e38]] + [(a, b) for a in one + [3.0e38] for b in inf]
    ys.append([p[0] for p in pairs]); xs.append([p[1] for p in pairs])
    return _cat(*ys), _cat(*xs)


def qnormalize_f32(q):
    """rv::qnormalize in numpy float32, operation for operation (the CPU test checks it against the probe)."""
    q = np.asarray(q, F)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    inv = F(1) / n
    return q * inv[:, None]


def euler_to_quat_f64(e):
    """Static-xyz Euler angles -> xyzw quaternion in double (the formula of transformations.py quaternion_from_euler,
    axes 'sxyz')."""
    e = np.asarray(e, np.float64)
    si, ci = np.sin(e[:, 0] / 2), np.cos(e[:, 0] / 2)
    sj, cj = np.sin(e[:, 1] / 2), np.cos(e[:, 1] / 2)
    sk, ck = np.sin(e[:, 2] / 2), np.cos(e[:, 2] / 2)
    return np.stack([si * cj * ck - ci * sj * sk, ci * sj * ck + si * cj * sk,
                     ci * cj * sk - si * sj * ck, ci * cj * ck + si * sj * sk], 1)


def rotation_angle(q1, q2):
    """Angle between two rotations given as xyzw quaternions, in double: both normalised here, then 2 asin of the norm
    of the vector part of q1 conj(q2) (2 acos of the dot product has a 6e-4 noise floor for float-born inputs)."""
    a = np.asarray(q1, np.float64); b = np.asarray(q2, np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True); b = b / np.linalg.norm(b, axis=1, keepdims=True)
    ax, ay, az, aw = a.T
    bx, by, bz, bw = -b[:, 0], -b[:, 1], -b[:, 2], b[:, 3]
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by - ax * bz + ay * bw + az * bx
    z = aw * bz + ax * by - ay * bx + az * bw
    return 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(x * x + y * y + z * z)))


def cos_pitch(q):
    """cy = cos(pitch) of a quaternion, in double: sqrt(m00^2 + m10^2) of the matrix of q normalised in double."""
    q = np.asarray(q, np.float64)
    x, y, z, w = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    return np.hypot(1 - 2 * (y * y + z * z), 2 * (x * y + w * z))


@functools.lru_cache(maxsize=None)
def random_quats():
    """2^18 random unit quaternions, drawn in double and rounded to float, NOT renormalised."""
    rng = np.random.default_rng(20246)
    q = rng.standard_normal((1 << 18, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)


@functools.lru_cache(maxsize=None)
def cube_quats():
    """The 24 rotations of the cube, one quaternion each (rounded to float, not renormalised)."""
    out = []
    for i in range(4):
        out.append([1.0 if j == i else 0.0 for j in range(4)])
    for s in range(8):
        out.append([0.5 if not (s >> j) & 1 else -0.5 for j in range(3)] + [0.5])
    r = math.sqrt(0.5)
    for i in range(4):
        for j in range(i + 1, 4):
            for sg in (1, -1):
                q = [0.0] * 4; q[i] = r; q[j] = sg * r
                out.append(q)
    q = np.array(out, np.float64)
    assert q.shape == (24, 4)
    return q.astype(F)


GIMBAL_PER_HALF_DECADE = 1 << 14


@functools.lru_cache(maxsize=None)
def gimbal_family():
    """(angles float64 [n, 3], quaternions float32 [n, 4]).  pitch = +-(pi/2 - d), d log-uniform in [1e-9, 1] with
    2^14 points in each of the 18 half-decades, then d = 0 exactly (256 points per sign); roll and yaw uniform in
    (-pi, pi).  The quaternion is built in double, rounded to float and put through the float qnormalize, as a body
    quaternion is after an integration step."""
    rng = np.random.default_rng(20247)
    m = GIMBAL_PER_HALF_DECADE
    u = np.concatenate([-9.0 + 0.5 * (h + rng.random(m)) for h in range(18)])
    d = np.concatenate([10.0 ** u, np.zeros(512)])
    sign = np.where(np.arange(d.size) % 2 == 0, 1.0, -1.0)
    e = np.stack([rng.uniform(-math.pi, math.pi, d.size), sign * (math.pi / 2 - d),
                  rng.uniform(-math.pi, math.pi, d.size)], 1)
    return e, qnormalize_f32(euler_to_quat_f64(e).astype(F))


@functools.lru_cache(maxsize=None)
def quats_raw():
    return np.concatenate([random_quats(), cube_quats(), gimbal_family()[1]])


@functools.lru_cache(maxsize=None)
def quats_unit():
    """The quaternions the Euler functions and the rotation tests see: all sets after the float qnormalize (the
    gimbal family has been through it already)."""
    return np.concatenate([qnormalize_f32(random_quats()), qnormalize_f32(cube_quats()), gimbal_family()[1]])


@functools.lru_cache(maxsize=None)
def euler_inputs():
    """Angles for euler_to_quat: the gimbal family rounded to float, and 2^16 triples uniform in (-pi, pi)."""
    rng = np.random.default_rng(20248)
    return np.concatenate([gimbal_family()[0], rng.uniform(-math.pi, math.pi, (1 << 16, 3))]).astype(F)


@functools.lru_cache(maxsize=None)
def vectors(n, seed):
    """n vectors: normal directions with lengths 10^u, u uniform in [-3, 3]."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(F)


# ---- Philox4x32-10
PHILOX_KAT = (      # Random123 known-answer vectors: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox_python(ctr, key):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11: ten rounds of two 32 x 32 -> 64 multiplications by
    0xD2511F53 / 0xCD9E8D57, key bumped by the golden-ratio / sqrt(3) Weyl constants): independent of both C sides."""
    m32 = 0xFFFFFFFF
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m32, (p0 >> 32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + 0x9E3779B9) & m32
        k1 = (k1 + 0xBB67AE85) & m32
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=None)
def philox_inputs():
    """The three known-answer (counter, key) pairs first, then 2^16 random pairs."""
    rng = np.random.default_rng(20249)
    ctr = rng.integers(0, 1 << 32, (1 << 16, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (1 << 16, 2), dtype=np.uint64).astype(np.uint32)
    ctr = np.concatenate([np.array([k[0] for k in PHILOX_KAT], np.uint32), ctr])
    key = np.concatenate([np.array([k[1] for k in PHILOX_KAT], np.uint32), key])
    return ctr, key


RNG_K = 16


@functools.lru_cache(maxsize=None)
def rng_inputs():
    """(seeds [n, 5] u32, lo [n], hi [n], randint n [n]): 2^14 streams of RNG_K draws (four Philox blocks each)."""
    rng = np.random.default_rng(20250)
    n = 1 << 14
    seeds = rng.integers(0, 1 << 32, (n, 5), dtype=np.uint64).astype(np.uint32)
    seeds[:64, 2:] = np.arange(64 * 3).reshape(64, 3)            # small gid / stream / arg, as the envs use them
    lo = rng.uniform(-10, 10, n).astype(F)
    hi = (lo + (10.0 ** rng.uniform(-6, 2, n)).astype(F)).astype(F)
    lo[:16], hi[:16] = 1.0, 2.0
    nmax = np.array(RANDINT_N, np.int32)[np.arange(n) % len(RANDINT_N)]
    return seeds, lo, hi, nmax


@functools.lru_cache(maxsize=None)
def cases():
    """name of the probe function -> (inputs, k)."""
    s = scalars()
    qa, qu = quats_raw(), quats_unit()
    rng = np.random.default_rng(20251)
    mats = np.concatenate([rng.uniform(-2, 2, (1 << 16, 9)).astype(F),
                           (rng.standard_normal((1 << 12, 9)) * 10.0 ** rng.uniform(-20, 20, (1 << 12, 1))).astype(F)])
    mv = vectors(mats.shape[0], 7)
    seeds, lo, hi, nmax = rng_inputs()
    both = np.concatenate([random_quats(), qu])                  # raw and normalised random sets, cube, gimbal family
    qb = qu[_perm(np.arange(qu.shape[0]), 5)]
    c = {
        'p_fsqrtr': ((sqrt_inputs(),), 1), 'p_frintr': ((s,), 1), 'p_ffloorr': ((s,), 1),
        'p_fclamp_pm': (clamp_pairs(), 1), 'p_fclampr_pm': (clamp_pairs(), 1),
        'p_fdiv': (division_pairs(), 1), 'p_frcp': ((s,), 1), 'p_fma': (fma_triples(), 1),
        'p_sincosr': ((sincos_inputs(),), 1), 'p_atan_pos': ((atan_pos_inputs(),), 1), 'p_atan2r': (atan2_inputs(), 1),
        'p_qmul': ((qa, qb), 1),
        'p_qnormalize': ((qa,), 1),
        'p_qrotv': ((both, vectors(both.shape[0], 6)), 1),
        'p_qmat': ((both,), 1), 'p_qaxis_z': ((both,), 1),
        'p_mulv': ((mats, mv), 1), 'p_tmulv': ((mats, mv), 1), 'p_mulv_mem': ((mats, mv), 1), 'p_tmulv_mem': ((mats, mv), 1),
        'p_euler_to_quat': ((euler_inputs(),), 1),
        'p_quat_to_euler': ((both,), 1), 'p_quat_yaw': ((both,), 1),
        'p_philox': (philox_inputs(), 1),
        'p_rng_uniform01': ((seeds,), RNG_K), 'p_rng_uniform': ((seeds, lo, hi), RNG_K),
        'p_rng_randint': ((seeds, nmax), RNG_K),
    }
    return c
