"""The scalar primitives of robovat_amd/csrc/rv_dev_math.h, called directly (tests/probe).

Every GPU parity test compares HIP with the float C oracle, and oracle/orc_math.h is a copy of rv_dev_math.h: a wrong
coefficient or threshold is wrong on both sides at once.  Here the header is compiled for the host and

* compared bit for bit with the float oracle over the shared inputs of tests/probe/inputs.py (the same inputs the
  device probe sees in tests/test_gpu_math_primitives.py), and
* measured against float64: libm and double quaternion algebra (the ORC_DOUBLE build of the probe), numpy's correctly
  rounded float32 sqrt and division, and a Philox written on Python integers.

The accuracy bounds are those of the primitives' contracts (rv_dev_math.h, DESIGN.md "device math"); each assertion
message carries the measured maximum.
"""
import math

import numpy as np
import pytest

from probe import build as probe_build, inputs

F = np.float32


@pytest.fixture(scope='module')
def host():
    return probe_build.host_probe()


@pytest.fixture(scope='module')
def orc32():
    return probe_build.oracle_probe(False)


@pytest.fixture(scope='module')
def orc64():
    return probe_build.oracle_probe(True)


_RESULTS = {}


def host_result(host, name):
    """The host compile's output for the shared case `name`: computed once, never modified."""
    if name not in _RESULTS:
        ins, k = inputs.cases()[name]
        r = host.call(name, *ins, k=k)
        r.setflags(write=False)
        _RESULTS[name] = r
    return _RESULTS[name]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32) if a.dtype == np.int32 else a


def first_difference(name, ins, got, want):
    """None, or a message that names the first differing element, its inputs and both outputs in hex."""
    g, w = bits(got).reshape(len(got), -1), bits(want).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(1))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    hexes = lambda row: ' '.join('%08x' % int(v) for v in row)      # noqa: E731
    shown = ['in%d = %s (%s)' % (j, np.asarray(x).reshape(len(got), -1)[i], hexes(bits(np.ascontiguousarray(np.asarray(x).reshape(len(got), -1)[i]))))
             for j, x in enumerate(ins)]
    return '%s: %d of %d elements differ; first at %d: %s; got %s, want %s' % (name, bad.size, len(got), i, ', '.join(shown), hexes(g[i]), hexes(w[i]))


@pytest.mark.parametrize('name', sorted(probe_build.FUNCS))
def test_host_compile_equals_float_oracle_bit_for_bit(host, orc32, name):
    """rv_dev_math.h (host compile) == oracle/orc_math.h (float), as uint32 words: -0 is not +0."""
    ins, k = inputs.cases()[name]
    got = host_result(host, name)
    want = orc32.call(name, *ins, k=k)
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.dtype == np.float32:
        assert not np.isnan(got).any(), '%s: the shared inputs must not produce a NaN' % name
    msg = first_difference(name, ins, got, want)
    assert msg is None, msg


def test_inputs_are_deterministic_and_nan_free():
    c = inputs.cases()
    assert set(c) == set(probe_build.FUNCS)
    for name, (ins, k) in c.items():
        for x in ins:
            if x.dtype.kind == 'f':
                assert not np.isnan(x).any(), name
    inputs.scalars.cache_clear()
    again = inputs.scalars()
    assert np.array_equal(again.view(np.uint32), c['p_frintr'][0][0].view(np.uint32))
    # what the generator promises about the scalars
    s = set(c['p_frintr'][0][0].view(np.uint32).tolist())
    for v in [0.0, -0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** 127, float(inputs.DEN_MAX), float(inputs.FLT_MAX), 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24]:
        assert int(F(v).view(np.uint32)) in s, v
    e, q = inputs.gimbal_family()
    d = math.pi / 2 - np.abs(e[:, 1])
    for h in range(18):
        lo, hi = 10.0 ** (-9 + 0.5 * h), 10.0 ** (-9 + 0.5 * (h + 1))
        assert ((d >= lo * (1 - 1e-6)) & (d < hi)).sum() >= (1 << 14) - 8, h     # (d is recovered from pitch: a few fall over an edge)
    assert (d == 0).sum() == 512
    # the generator's numpy qnormalize is the header's
    assert inputs.qnormalize_f32(inputs.random_quats()).dtype == np.float32


def test_numpy_qnormalize_is_the_headers(host):
    raw = np.concatenate([inputs.random_quats(), inputs.cube_quats()])
    got = host.call('p_qnormalize', raw)
    assert np.array_equal(got.view(np.uint32), inputs.qnormalize_f32(raw).view(np.uint32))


# ---------------------------------------------------------------- correctly rounded operations

def test_sqrt_and_division_are_correctly_rounded(host):
    """fsqrtr, a / b and 1.0f / a equal numpy.float32 sqrt and division (correctly rounded) bit for bit: denormal
    inputs and results and exact ties included."""
    with np.errstate(all='ignore'):
        (x,), _ = inputs.cases()['p_fsqrtr']
        msg = first_difference('fsqrtr', (x,), host_result(host, 'p_fsqrtr'), np.sqrt(x))
        assert msg is None, msg
        (a, b), _ = inputs.cases()['p_fdiv']
        q = host_result(host, 'p_fdiv')
        msg = first_difference('a / b', (a, b), q, a / b)
        assert msg is None, msg
        # numpy's float32 division against the quotient in double rounded once more: equal except where that double
        # rounding itself is wrong, which it is not for these operand widths (53 >= 2 * 24 + 2)
        assert np.array_equal(q.view(np.uint32), (a.astype(np.float64) / b.astype(np.float64)).astype(F).view(np.uint32))
        den = (np.abs(q) > 0) & (np.abs(q) < inputs.FLT_MIN)
        assert den.sum() > 1 << 16, 'the pairs with a denormal quotient are missing'
        (s,), _ = inputs.cases()['p_frcp']
        msg = first_difference('1.0f / a', (s,), host_result(host, 'p_frcp'), F(1) / s)
        assert msg is None, msg


def test_rint_floor_fma(host):
    """frintr rounds ties to even, ffloorr is floor, rv_fma has ONE rounding (the product is not rounded first)."""
    (s,), _ = inputs.cases()['p_frintr']
    assert np.array_equal(host_result(host, 'p_frintr').view(np.uint32), np.rint(s).view(np.uint32))
    assert np.array_equal(host_result(host, 'p_ffloorr').view(np.uint32), np.floor(s).view(np.uint32))
    ties = np.arange(-64, 65, dtype=np.float64) + 0.5
    r = host.call('p_frintr', ties.astype(F))
    assert (r % 2 == 0).all() and (np.abs(r - ties) == 0.5).all()
    (a, b, c), _ = inputs.cases()['p_fma']
    with np.errstate(all='ignore'):
        exact = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        # (double holds the product exactly; the sum is rounded to double and then to float: a double rounding that
        # can differ from the single one only at a tie of the second -- compared where it cannot)
        want = exact.astype(F)
        got = host_result(host, 'p_fma')
        ok = np.isfinite(exact)
        differ = (got.view(np.uint32) != want.view(np.uint32)) & ok
        # a difference must be a double-rounding case: within one float ulp and with `exact` on a float tie
        if differ.any():
            lo = np.minimum(got[differ], want[differ]).astype(np.float64); hi = np.maximum(got[differ], want[differ]).astype(np.float64)
            assert (np.nextafter(lo.astype(F), F(np.inf)).astype(np.float64) == hi).all() and (exact[differ] == (lo + hi) / 2).all()
    # the cancellation block: c = -round(a b), so the fused result is the product's rounding error, exactly
    n2 = 1 << 16
    a2, b2, c2 = a[-n2:].astype(np.float64), b[-n2:].astype(np.float64), c[-n2:].astype(np.float64)
    assert np.array_equal(got[-n2:].astype(np.float64), a2 * b2 + c2)
    assert (got[-n2:] != 0).mean() > 0.5


def test_fclamp_pm_is_fclampr(host):
    """fclamp_pm(x, b) == fclampr(x, -b, b) for every non-NaN x and every b > 0 (denormal b, +-0 and +-inf as x)."""
    (x, b), _ = inputs.cases()['p_fclamp_pm']
    assert (b > 0).all() and (b < inputs.FLT_MIN).sum() > 1000 and np.isinf(x).sum() >= 2
    got, ref = host_result(host, 'p_fclamp_pm'), host_result(host, 'p_fclampr_pm')
    msg = first_difference('fclamp_pm', (x, b), got, ref)
    assert msg is None, msg
    want = np.where(x < -b, -b, np.where(x > b, b, x))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- sincos / atan2 against libm in double

def _ulp_of(t):
    """One float ulp at the magnitude of the double t."""
    return np.spacing(np.maximum(np.abs(t), float(inputs.DEN_MIN)).astype(F)).astype(np.float64)


def _sincos_errors(host, orc64):
    (x,), _ = inputs.cases()['p_sincosr']
    got = host_result(host, 'p_sincosr').astype(np.float64)
    want = orc64.call('p_sincosr', x)
    assert np.abs(want - np.stack([np.sin(x.astype(np.float64)), np.cos(x.astype(np.float64))], 1)).max() < 1e-15     # libm == numpy
    return x, got, want, np.abs(got - want)


def test_sincosr_absolute_accuracy(host, orc64):
    """|error| <= 2^-23 (one float ulp of 1) on the whole domain |x| <= 1e4."""
    x, got, want, err = _sincos_errors(host, orc64)
    worst = err.max()
    i = int(err.max(1).argmax())
    print('sincosr: max abs error %.3e at x = %r over |x| <= 1e4 (%d points)' % (worst, float(x[i]), x.size))
    assert worst <= 2.0 ** -23, 'sincosr: max abs error %.3e at x = %r (bound 2^-23 = 1.19e-7)' % (worst, float(x[i]))
    # exact facts; sin(-0) is +0 (the reduction computes -0 - (-0 * C1) = +0): pinned, not IEEE's -0
    z = host.call('p_sincosr', np.array([0.0, -0.0], F))
    assert np.array_equal(z.view(np.uint32), np.array([[0.0, 1.0], [0.0, 1.0]], F).view(np.uint32))
    den = np.abs(x) < inputs.FLT_MIN
    assert np.array_equal(got[den, 0], x[den].astype(np.float64)) and (got[den, 1] == 1).all()      # sin x = x, denormals kept
    # sin^2 + cos^2
    assert np.abs(got[:, 0] ** 2 + got[:, 1] ** 2 - 1).max() <= 4 * 2.0 ** -23


def test_sincosr_relative_accuracy_to_26(host, orc64):
    """<= 2 ulp of the true value on |x| <= 26, the floats next to the multiples of pi/2 included.  With the plain
    three-term reduction this held on the uniform sweep (1.54 ulp) but the floats of +-3 pi/2, +-3 pi and +-6 pi were
    off by 13.8 ulp (a cosine of 1.19e-8 wrong by 1.2e-14: k * C3 is rounded, and C3 is pi/2 - C1 - C2 only to
    1.7e-15); sincosr now redoes the last reduction step with fused multiply-adds and a fourth term wherever the
    reduced argument is below 2^-16."""
    x, got, want, err = _sincos_errors(host, orc64)
    near = np.abs(x) <= 26
    assert near.sum() > 1 << 20
    ulps = (err / _ulp_of(want))[near]
    sweep = ulps[:1 << 20]                    # (the uniform sweep of |x| <= 26 comes first in the inputs)
    print('sincosr: max error %.3f ulp of the true value over the uniform sweep of |x| <= 26' % sweep.max())
    j = int(ulps.max(1).argmax())
    print('sincosr: max error %.3f ulp of the true value at x = %r over all inputs with |x| <= 26' % (ulps.max(), float(x[near][j])))
    assert ulps.max() <= 2.0, 'sincosr: %.3f ulp at x = %r (bound 2 ulp on |x| <= 26)' % (ulps.max(), float(x[near][j]))


def test_atan2r_accuracy_sign_and_quadrant(host, orc64):
    """|error| <= 4e-7 (about 1.5 ulp of pi) against libm atan2 wherever y != 0; sign and quadrant exact wherever both
    components are finite and non-zero; the values at zeros and infinities pinned."""
    (y, x), _ = inputs.cases()['p_atan2r']
    got = host_result(host, 'p_atan2r')
    want = orc64.call('p_atan2r', y, x)
    assert np.abs(want - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 1e-15                        # libm == numpy
    # y = +-0 is excluded from the comparison, not from the inputs: atan2r ignores the sign of a zero y (pinned below)
    m = y != 0
    err = np.abs(got.astype(np.float64) - want)[m]
    i = int(err.argmax())
    print('atan2r: max abs error %.3e at (y, x) = (%r, %r), %d points' % (err.max(), float(y[m][i]), float(x[m][i]), m.sum()))
    assert err.max() <= 4e-7, 'atan2r: max abs error %.3e at (y, x) = (%r, %r) (bound 4e-7)' % (err.max(), float(y[m][i]), float(x[m][i]))
    reg = np.isfinite(y) & np.isfinite(x) & (y != 0) & (x != 0)
    assert reg.sum() > 1 << 20
    half_pi = F(1.5707963267948966)
    assert np.array_equal(np.signbit(got[reg]), np.signbit(y[reg])), 'sign of atan2r != sign of y'
    a = np.abs(got[reg])
    assert (a[x[reg] > 0] <= half_pi).all() and (a[x[reg] < 0] >= half_pi).all() and (a <= F(math.pi)).all()
    # pinned: a zero y is +0 whatever its sign (libm: -0 -> -pi / -0); x = +-0 is the y axis; inf / inf is not an input
    pin = {(0.0, 1.0): 0.0, (-0.0, 1.0): 0.0, (0.0, -1.0): math.pi, (-0.0, -1.0): math.pi,
           (0.0, 0.0): 0.0, (-0.0, -0.0): 0.0, (0.0, -0.0): 0.0, (1.0, 0.0): math.pi / 2, (1.0, -0.0): math.pi / 2,
           (-1.0, 0.0): -math.pi / 2, (1.0, -float(inputs.DEN_MIN)): math.pi / 2, (np.inf, 1.0): math.pi / 2,
           (-np.inf, -1.0): -math.pi / 2, (1.0, np.inf): 0.0, (1.0, -np.inf): math.pi, (-1.0, -np.inf): -math.pi}
    py = np.array([p[0] for p in pin], F); px = np.array([p[1] for p in pin], F)
    r = host.call('p_atan2r', py, px)
    assert np.array_equal(r.view(np.uint32), np.array(list(pin.values()), np.float64).astype(F).view(np.uint32)), r


def test_atan_pos_accuracy(host, orc64):
    """atan_pos (x >= 0, +inf included) within 4e-7 of libm atan: the thresholds +-2 ulp are in the inputs."""
    (x,), _ = inputs.cases()['p_atan_pos']
    err = np.abs(host_result(host, 'p_atan_pos').astype(np.float64) - orc64.call('p_atan_pos', x))
    print('atan_pos: max abs error %.3e at x = %r' % (err.max(), float(x[int(err.argmax())])))
    assert err.max() <= 4e-7, (err.max(), float(x[int(err.argmax())]))


# ---------------------------------------------------------------- quaternion algebra against double

def test_qnormalize_norm(host):
    """| ||q|| - 1 | <= 2^-22 after qnormalize (norm taken in double), for the raw sets and the gimbal family."""
    q = np.concatenate([host_result(host, 'p_qnormalize'), inputs.quats_unit()]).astype(np.float64)
    dev = np.abs(np.linalg.norm(q, axis=1) - 1)
    print('qnormalize: max | ||q|| - 1 | = %.3e' % dev.max())
    assert dev.max() <= 2.0 ** -22, 'qnormalize: max | ||q|| - 1 | = %.3e (bound 2^-22 = 2.38e-7)' % dev.max()


def test_rotations_agree_with_double(host, orc64):
    """qrotv(q, v) and qmat(q) v against the same expressions in double on the same float q: every component within
    8 2^-24 ||v||.  (Per component: each is a separately rounded float, and the bound counts its roundings in ulps of
    the vector's length -- about 4 products and 4 sums of magnitude <= ||v||, twice for the nested cross product.)"""
    (q, v), _ = inputs.cases()['p_qrotv']
    vn = np.linalg.norm(v.astype(np.float64), axis=1)
    want = orc64.call('p_qrotv', q, v)
    e1 = np.abs(host_result(host, 'p_qrotv').astype(np.float64) - want).max(1) / vn
    m = host_result(host, 'p_qmat')
    assert m.shape[0] == q.shape[0]
    e2 = np.abs(host.call('p_mulv', m, v).astype(np.float64) - want).max(1) / vn
    e3 = np.abs(host.call('p_tmulv_mem', m, host.call('p_mulv_mem', m, v)).astype(np.float64) - v.astype(np.float64)).max(1) / vn
    print('qrotv: %.2f, qmat mulv: %.2f, tmulv(mulv): %.2f (units of 2^-24 ||v||)' % (e1.max() * 2 ** 24, e2.max() * 2 ** 24, e3.max() * 2 ** 24))
    assert e1.max() <= 8 * 2.0 ** -24, 'qrotv: %.2f x 2^-24 ||v|| (bound 8)' % (e1.max() * 2 ** 24)
    assert e2.max() <= 8 * 2.0 ** -24, 'qmat mulv: %.2f x 2^-24 ||v|| (bound 8)' % (e2.max() * 2 ** 24)
    # qaxis_z is the third column of qmat, same expressions
    assert np.array_equal(host_result(host, 'p_qaxis_z').view(np.uint32), np.ascontiguousarray(m[:, [2, 5, 8]]).view(np.uint32))
    # qmul against double
    (a, b), _ = inputs.cases()['p_qmul']
    e4 = np.abs(host_result(host, 'p_qmul').astype(np.float64) - orc64.call('p_qmul', a, b)).max()
    assert e4 <= 4 * 2.0 ** -24, e4


def test_cube_rotations_are_exact_permutations(host):
    """The 24 cube rotations: qmat of the normalised quaternion is a signed permutation matrix to within 2^-22, the 24
    are distinct, and quat_to_euler -> euler_to_quat returns the same rotation."""
    q = host.call('p_qnormalize', inputs.cube_quats())
    m = host.call('p_qmat', q).astype(np.float64)
    r = np.rint(m)
    assert np.abs(m - r).max() <= 2.0 ** -22
    assert (np.abs(r).reshape(24, 3, 3).sum(1) == 1).all() and (np.abs(r).reshape(24, 3, 3).sum(2) == 1).all()
    assert np.allclose(np.linalg.det(r.reshape(24, 3, 3)), 1.0)
    assert len({tuple(row) for row in r.tolist()}) == 24


def test_euler_to_quat_against_double(host, orc64):
    """euler_to_quat on the gimbal family and on uniform angles: within 1e-6 rad of the double conversion of the same
    float angles."""
    (e,), _ = inputs.cases()['p_euler_to_quat']
    want = orc64.call('p_euler_to_quat', e)
    assert np.abs(want - inputs.euler_to_quat_f64(e)).max() < 1e-15
    err = inputs.rotation_angle(host_result(host, 'p_euler_to_quat'), want)
    print('euler_to_quat: max rotation error %.3e rad' % err.max())
    assert err.max() <= 1e-6, 'euler_to_quat: max rotation error %.3e rad at angles %s (bound 1e-6)' % (err.max(), e[int(err.argmax())])


def euler_bound(cy):
    """The rotation error allowed to quat_to_euler: 16 float ulps of 1 over cos(pitch) in the regular branch, capped
    at 2e-3 (about 5 sqrt(eps_float)) across gimbal lock, plus 4e-6 for the three atan2r and the float input."""
    with np.errstate(divide='ignore'):
        return np.minimum(2e-3, 16 * 2.0 ** -23 / cy) + 4e-6


def euler_round_trip_error(q, angles):
    """Angle between the rotation of the float quaternion q (taken to double and normalised there) and the rotation
    rebuilt IN DOUBLE from the float Euler angles."""
    return inputs.rotation_angle(inputs.euler_to_quat_f64(np.asarray(angles, np.float64)), q)


def test_quat_to_euler_round_trip(host):
    """Every quaternion of the gimbal family, the random sets and the cube rotations: the rotation rebuilt in double
    from the angles quat_to_euler returns is within min(2e-3, 16 2^-23 / cy) + 4e-6 rad of the input rotation, cy =
    cos(pitch) of the input in double.  No case is exempt.  With the reference's float64-sized gimbal threshold (1e-6)
    carried over to float this fails by a factor of 205 (0.41 rad at cy = 1.2e-6); the float threshold is 3e-4."""
    (q,), _ = inputs.cases()['p_quat_to_euler']
    e = host_result(host, 'p_quat_to_euler')
    assert np.isfinite(e).all()
    err = euler_round_trip_error(q, e)
    cy = inputs.cos_pitch(q)
    ratio = err / euler_bound(cy)
    i = int(ratio.argmax())
    print('quat_to_euler: worst error / bound = %.3f (error %.3e rad at cy = %.3e); max error %.3e rad' % (ratio[i], err[i], cy[i], err.max()))
    for lo, hi in ((0, 1e-6), (1e-6, 1e-5), (1e-5, 1e-4), (1e-4, 3.2e-4), (3.2e-4, 1e-3), (1e-3, 1e-2), (1e-2, 2)):
        m = (cy >= lo) & (cy < hi)
        if m.any():
            print('  cy in [%.1e, %.1e): %7d quaternions, max error %.3e rad' % (lo, hi, m.sum(), err[m].max()))
    assert (cy < 3e-4).sum() > 1000 and ((cy >= 3e-4) & (cy < 1e-3)).sum() > 1000, 'the gimbal family misses the band'
    assert ratio[i] <= 1.0, ('quat_to_euler: rotation error %.3e rad at cy = %.3e, q = %s, angles %s: %.1f x the bound'
                             % (err[i], cy[i], q[i], e[i], ratio[i]))
    # pitch stays in [-pi/2, pi/2] and yaw is exactly 0 in the lock branch
    assert (np.abs(e[:, 1]) <= F(1.5707963267948966)).all()
    # quat_yaw is the yaw of the regular branch (same expression): equal bits wherever that branch was taken
    yaw = host_result(host, 'p_quat_yaw')
    regular = cy > 1e-3
    assert np.array_equal(yaw[regular].view(np.uint32), e[regular, 2].view(np.uint32))


# ---------------------------------------------------------------- Philox and the streams

def test_philox_known_answers_and_python_integers(host):
    """The three Random123 known-answer vectors, then 2^16 random (counter, key) pairs against Philox4x32-10 on Python
    integers (inputs.philox_python: written for this test, shares nothing with the C sides)."""
    for ctr, key, out in inputs.PHILOX_KAT:
        assert inputs.philox_python(ctr, key) == out
    ctr, key = inputs.philox_inputs()
    got = host_result(host, 'p_philox')
    assert got.dtype == np.uint32
    for j, (_, _, out) in enumerate(inputs.PHILOX_KAT):
        assert tuple(int(v) for v in got[j]) == out, (j, [hex(int(v)) for v in got[j]])
    want = np.array([inputs.philox_python([int(v) for v in c], [int(v) for v in k]) for c, k in zip(ctr.tolist(), key.tolist())], np.uint64).astype(np.uint32)
    assert np.array_equal(got, want)


def test_rng_streams(host):
    """rng_init / rng_u32 walk the Philox blocks of counter (j, arg, gid, stream) under key (seed_lo, seed_hi);
    rng_uniform01 is in [0, 1) on a 2^-24 grid; rng_randint(n) < n; rng_uniform(lo, hi) stays in [lo, hi] -- and CAN
    return hi, by rounding (the behaviour is pinned, not changed)."""
    seeds, lo, hi, nmax = inputs.rng_inputs()
    k = inputs.RNG_K
    u = host_result(host, 'p_rng_uniform01')
    assert u.shape == (seeds.shape[0], k)
    assert (u >= 0).all() and (u < 1).all() and (u * 2.0 ** 24 == np.rint(u * 2.0 ** 24)).all()
    # the words behind the draws, from the Python-integer Philox, for the first streams
    for i in range(32):
        s = [int(v) for v in seeds[i]]
        words = []
        for j in range(k // 4):
            words += inputs.philox_python((j, s[4], s[2], s[3]), (s[0], s[1]))
        assert np.array_equal(u[i], (np.array(words, np.uint64) >> 8).astype(F) * F(2.0 ** -24)), i
    assert abs(float(u.mean()) - 0.5) < 0.01
    r = host_result(host, 'p_rng_randint')
    assert (r >= 0).all() and (r < nmax[:, None]).all()
    for n in inputs.RANDINT_N:
        rows = r[nmax == n]
        assert rows.size > 1000
        if n <= 64:
            assert set(np.unique(rows).tolist()) == set(range(n)), n
    v = host_result(host, 'p_rng_uniform')
    assert np.array_equal(v.view(np.uint32), (lo[:, None] + (hi - lo)[:, None] * u).view(np.uint32))
    assert (v >= lo[:, None]).all() and (v <= hi[:, None]).all()
    # it can return hi: the largest draw u = 1 - 2^-24 between lo = 1 and hi = 2 gives 2 - 2^-24, a tie that rounds to 2
    umax = F(1) - F(2.0 ** -24)
    assert umax == F((2 ** 24 - 1) * 2.0 ** -24) and F(1) + (F(2) - F(1)) * umax == F(2)
