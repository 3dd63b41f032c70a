"""rv_dev_collide.h and the cross-lane primitives of rv_dev_wave.h on the MI355X (tests/probe/rv_collide_probe.hip, compiled
for gfx950 with exactly the product's flags by __graft_entry__.build()).

* Device equals host, bit for bit: support_v, the sub-simplex solvers, gjk_epa (every output word, lb_out and the simplex
  cache included), man_add and plane_space over every input class of tests/test_collide_probe.py, which holds the host
  compile to float64.  The one exception is the sign of a zero support_v PROJECTION (rv_dev_wave.h row_ror_fmax), compared
  with ==.  Items of different classes and vertex counts are interleaved, so the four rows of a wave differ; launches
  hold at most 1023 items (256 blocks of one wave, the last with one padded group).
* Row steps: out[lane] = op(x[lane], x[source(lane)]) with source(lane) = 16 * row + ((lane - N) mod 16): the DPP control
  row_ror:N rotates the row RIGHT, towards higher lane numbers, so lane l receives the value of the lane N below it,
  wrapping within its own row of 16 (AMD "CDNA3/CDNA4 Instruction Set Architecture", DPP_ROW_RR; the guides shipped with
  this project do not restate it).  The same for every row_ror_* primitive and grp_ror_max.  grp_bcast<S> gives lane
  16 * row + S to its row.
* The 8, 4, 2, 1 all-reduces against numpy; fmax on finite inputs with denormals, signed zeros, equal values.
* wave_min / wave_max / rdlane / unif against numpy over 64 lanes.

Every output array lies between guard words that must come back untouched (probe_build.CollideProbe checks them on
every call).  A missing or stale device probe is an error, never a skip.
"""
import numpy as np
import pytest

from probe import build as probe_build, collide_inputs as ci
from test_collide_probe import CONCENTRIC_SEED, mirror_pairs

pytestmark = pytest.mark.gpu
F = np.float32
CHUNK = 1023                  # items per launch: not a multiple of 4


@pytest.fixture(scope='module')
def device():
    return probe_build.CollideProbe(device=True)


@pytest.fixture(scope='module')
def host():
    return probe_build.CollideProbe()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def both(device, host, name, *arrays):
    """the export on both builds, in launches of CHUNK items -> (device outputs, host outputs)"""
    n = len(arrays[0])
    want = host.call(name, *arrays)
    got = [device.call(name, *[a[s:s + CHUNK] for a in arrays]) for s in range(0, n, CHUNK)]
    return tuple(np.concatenate([g[k] for g in got]) for k in range(len(want))), want


def assert_same_words(name, got, want, labels):
    for g, w, label in zip(got, want, labels):
        assert g.dtype == w.dtype and g.shape == w.shape
        bad = np.nonzero((bits(g) != bits(w)).reshape(len(g), -1).any(1))[0]
        assert bad.size == 0, '%s %s: %d of %d items differ, first %d: device %s host %s' % (name, label, bad.size, len(g), bad[0], g[bad[0]], w[bad[0]])


# ------------------------------------------------------------------------------------------------- device equals host --
def test_support_v_equals_host(device, host):
    verts, cnt, dirs, tags = ci.support_cases()
    if len(cnt) % 4 == 0:                       # leave a padded group in the last wave
        verts, cnt, dirs = verts[:-1], cnt[:-1], dirs[:-1]
    # consecutive items (the rows of one wave) hold different counts
    distinct = np.array([len(set(q)) for q in cnt[:len(cnt) // 4 * 4].reshape(-1, 4)])
    assert (distinct >= 2).mean() > 0.9 and (distinct == 4).sum() >= 8
    (proj, idx, v, proj2), (hproj, hidx, hv, hproj2) = both(device, host, 'c_support_v', verts, cnt, dirs)
    assert_same_words('support_v', (idx, v), (hidx, hv), ('index', 'vertex'))
    # the projection: the maximum itself, up to the sign of a zero
    assert np.array_equal(proj, hproj) and np.array_equal(proj2, hproj2)
    nz = hproj[:, 0] != 0
    assert np.array_equal(bits(proj)[nz], bits(hproj)[nz]) and np.array_equal(bits(proj2)[nz], bits(hproj2)[nz])


def test_sub_simplex_solvers_equal_host(device, host):
    W2, W3, W4 = ci.simplex_cases(2), ci.simplex_cases(3), ci.simplex_cases(4)
    got, want = both(device, host, 'c_closest_segment', W2.reshape(len(W2), 6))
    assert_same_words('closest_segment', got, want, ('weights',))
    got, want = both(device, host, 'c_closest_triangle', W3.reshape(len(W3), 9))
    assert_same_words('closest_triangle', got, want, ('weights',))
    # simplex_weights: every size in one array, interleaved
    Ws, ns = [], []
    for nv, W in ((4, W4), (3, W3), (2, W2), (1, W2)):
        P = np.zeros((len(W), 4, 3), F); P[:, :W.shape[1]] = W
        Ws.append(P.reshape(len(W), 12)); ns.append(np.full(len(W), nv, np.int32))
    Ws, ns = np.concatenate(Ws), np.concatenate(ns)
    order = np.random.RandomState(5).permutation(len(ns))
    got, want = both(device, host, 'c_simplex_weights', Ws[order], ns[order])
    assert_same_words('simplex_weights', got, want, ('weights', 'inside'))
    assert want[1].sum() >= 30


def _gjk_batches(host):
    """Every CPU class as argument arrays of c_gjk_epa: uncached, with an empty cache, misses at half the distance, the
    moved pairs with the cache their first query left and with stale / foreign caches."""
    batches = []
    for cls in ci.GJK_CLASSES:
        for ov in (False, True):
            batches.append(ci.gjk_arrays(ci.gjk_pairs(cls, ov)))
        sep = ci.gjk_pairs(cls, False)
        batches.append(ci.gjk_arrays(sep, use_gc=1, pair_id=3))
        hit, res, _ = host.call('c_gjk_epa', *ci.gjk_arrays(sep))
        batches.append(ci.gjk_arrays(sep, max_dist=(0.5 * np.abs(res[:, 3])).astype(F)))
    batches.append(ci.gjk_arrays(ci.concentric_pairs(CONCENTRIC_SEED)))
    mirror = mirror_pairs()[0]                       # the touching and mirror-symmetric cases, repeated to a batch
    batches.append(ci.gjk_arrays((mirror * (ci.PAIRS_PER_CLASS // len(mirror) + 1))[:ci.PAIRS_PER_CLASS], use_gc=1, pair_id=2))
    for cls in ('random', 'boxes', 'cylinders', 'parallel'):
        pairs, moved = ci.gjk_pairs(cls, False), ci.gjk_pairs('moved:' + cls, False)
        _, _, gc = host.call('c_gjk_epa', *ci.gjk_arrays(pairs, use_gc=1, pair_id=5))
        batches.append(ci.gjk_arrays(moved, use_gc=1, pair_id=5, gc=gc))
        batches.append(ci.gjk_arrays(moved, use_gc=1, pair_id=6, gc=gc))
        bad = gc.copy(); bad[:, 2] = [len(p[0]) for p in pairs]
        batches.append(ci.gjk_arrays(moved, use_gc=1, pair_id=5, gc=bad))
    batches = [batches[i] for i in np.random.RandomState(11).permutation(len(batches))]     # neighbours of different classes
    arrays = [np.concatenate([b[k] for b in batches]) for k in range(9)]
    # interleave: item i of every batch side by side, so that the rows of a wave hold different classes
    m = len(batches)
    order = np.arange(len(arrays[0])).reshape(m, -1).T.ravel()
    return [a[order] for a in arrays]


def test_gjk_epa_equals_host(device, host):
    arrays = _gjk_batches(host)
    n = len(arrays[0])
    assert n > 10000
    quads = (arrays[1] * 32 + arrays[3])[:n // 4 * 4].reshape(-1, 4)                       # the vertex counts of a wave's rows
    mixed = np.array([len(set(q)) for q in quads])
    print('waves whose rows hold 4 / 3 / 2 / 1 different vertex counts:', [(mixed == k).sum() for k in (4, 3, 2, 1)])
    assert (mixed >= 3).mean() > 0.8
    got, want = both(device, host, 'c_gjk_epa', *arrays)
    hit, res, gc = want
    # every path is in there: misses, separated hits, EPA hits, caches written and emptied
    assert (hit == 0).sum() > 1000 and ((hit[:, 0] == 1) & (res[:, 3] > 0)).sum() > 3000 and ((hit[:, 0] == 1) & (res[:, 3] < 0)).sum() > 2000
    assert (gc[:, 0] > 0).sum() > 1000
    assert_same_words('gjk_epa', got, want, ('hit', 'n dist pa pb lb_out', 'cache'))


def test_man_add_and_plane_space_equal_host(device, host):
    mans, pts, cols, _ = ci.man_add_cases()
    assert device.man_words == host.man_words == mans.shape[1]
    got, want = both(device, host, 'c_man_add', mans[:-1], pts[:-1], cols[:-1])       # 399 items: a padded group
    assert_same_words('man_add', got, want, ('manifold',))
    n = ci.plane_space_cases()
    got, want = both(device, host, 'c_plane_space', n)
    assert_same_words('plane_space', got, want, ('t1 t2',))


# ---------------------------------------------------------------------------------------------------------- row steps --
WAVES = 3


def source(N):
    """the lane whose value row_ror:N brings to each of the 64 lanes: N below, wrapping within the row of 16"""
    lane = np.arange(64)
    return (lane & ~15) | ((lane - N) & 15)


def row_values(seed):
    """[WAVES, 64] small integers, a different permutation of 16 distinct values in every row (scaled per row): a step that
    leaks across rows, or a step of another width, gives another answer"""
    rng = np.random.RandomState(seed)
    v = np.stack([(rng.permutation(16) - 7) * (r + 2) + (r % 3) for r in range(WAVES * 4)])
    return v.reshape(WAVES, 64)


@pytest.mark.parametrize('prim', ['row_ror_f', 'row_ror_i', 'row_ror_fmax', 'row_ror_imin', 'row_ror_min', 'row_ror_add', 'grp_ror_max'])
def test_row_step(device, prim):
    is_float = prim in ('row_ror_f', 'row_ror_fmax', 'row_ror_min', 'row_ror_add')
    for N in (1, 2, 4, 8):
        v = row_values(10 * N + len(prim))
        x = (v * 0.37).astype(F) if is_float else v.astype(np.int32)
        o = x[:, source(N)]
        want = {'row_ror_f': o, 'row_ror_i': o, 'row_ror_fmax': np.maximum(x, o), 'row_ror_imin': np.minimum(x, o),
                'row_ror_min': np.minimum(x, o), 'row_ror_add': (o + x).astype(x.dtype), 'grp_ror_max': np.maximum(x, o)}[prim]
        got, = device.call('c_row_step', bits(x), sel=(probe_build.ROW_PRIMS[prim], N))
        other = x[:, (np.arange(64) & ~15) | ((np.arange(64) + N) & 15)]
        assert np.array_equal(got, bits(want)), '%s<%d>: lane 0..15 of wave 0 gave %s from %s (the opposite rotation would bring %s)' % (
            prim, N, got[0, :16].view(x.dtype), x[0, :16], other[0, :16])


def test_grp_bcast(device):
    x = (row_values(99) * 1.25).astype(F)
    for S in range(16):
        got, = device.call('c_row_step', bits(x), sel=(probe_build.ROW_PRIMS['grp_bcast'], S))
        assert np.array_equal(got, bits(x[:, (np.arange(64) & ~15) | S])), S


# -------------------------------------------------------------------------------------------------------- all-reduces --
def fmax_rows():
    """[k, 16] finite float32 rows: large and tiny magnitudes, signed zeros, denormals, equal values"""
    rng = np.random.RandomState(7)
    tiny = np.float32(1e-45)
    rows = [rng.randn(16) * 10.0 ** rng.uniform(-30, 30) for _ in range(24)]
    rows += [10.0 ** rng.uniform(-37, 38, 16) * rng.choice([-1, 1], 16) for _ in range(16)]
    rows += [np.full(16, v) for v in (1.5, -2.0, 3.0e38, -3.0e38, 1.1754944e-38)]                     # equal values
    rows += [np.where(rng.rand(16) < 0.5, 0.0, -0.0) for _ in range(6)] + [np.full(16, -0.0), np.full(16, 0.0)]
    rows += [np.where(rng.rand(16) < 0.3, 0.0, -np.abs(rng.randn(16))) for _ in range(6)]            # a zero over negatives
    rows += [np.where(rng.rand(16) < 0.3, -0.0, -np.abs(rng.randn(16))) for _ in range(6)]
    den = [tiny * rng.randint(1, 1 << 22, 16) * rng.choice([-1, 1], 16) for _ in range(12)]          # denormals only
    den += [np.where(rng.rand(16) < 0.5, tiny * rng.randint(1, 1 << 22, 16), -np.abs(rng.randn(16))) for _ in range(6)]
    den += [-(tiny * rng.randint(1, 1 << 22, 16)) for _ in range(6)]                                  # negative denormals
    den += [np.where(rng.rand(16) < 0.5, -(tiny * rng.randint(1, 1 << 22, 16)), -0.0) for _ in range(4)]
    rows = np.asarray(rows + den, F)
    pad = (-len(rows)) % 4
    return np.concatenate([rows, rows[:pad]])


def test_fmax_allreduce_is_the_row_maximum_of_finite_inputs(device):
    """v_max_f32 on the rotated value equals the ternary's maximum on every finite input up to the sign of a zero.
    Denormals: the kernels are compiled with float32 denormals kept (the mode the product runs in), and the maximum
    of a row of denormals is that denormal, not a zero."""
    rows = fmax_rows()
    assert np.isfinite(rows).all()
    sub = (np.abs(rows) < np.float32(1.1754944e-38)) & (rows != 0)
    assert sub.any(1).sum() >= 20
    got, = device.call('c_row_allreduce', bits(rows).reshape(-1, 64), sel=(probe_build.REDUCE_PRIMS['fmax'],))
    got = got.view(F).reshape(-1, 16)
    want = rows.max(1, keepdims=True)                       # the ternary's value: the largest input (no NaN here)
    assert (got == got[:, :1]).all(), 'the lanes of a row disagree'
    assert np.array_equal(got[:, :1], want), (got[:, 0], want[:, 0])
    nz = want[:, 0] != 0
    assert np.array_equal(bits(got[:, 0])[nz], bits(want[:, 0])[nz])        # bits: a denormal maximum comes back as itself
    assert ((np.abs(want[:, 0]) < np.float32(1.1754944e-38)) & nz).sum() >= 16


def test_imin_min_add_allreduces(device):
    rng = np.random.RandomState(8)
    xi = rng.randint(-2 ** 31, 2 ** 31 - 1, (64, 16)).astype(np.int32)
    xi[:8] = rng.randint(-3, 3, (8, 16))                                          # ties
    got, = device.call('c_row_allreduce', bits(xi).reshape(-1, 64), sel=(probe_build.REDUCE_PRIMS['imin'],))
    assert np.array_equal(got.view(np.int32).reshape(-1, 16), np.repeat(xi.min(1, keepdims=True), 16, 1))
    xf = (rng.randn(64, 16) * 10.0 ** rng.uniform(-20, 20, (64, 1))).astype(F)
    xf[:8] = rng.randint(-3, 3, (8, 16))
    got, = device.call('c_row_allreduce', bits(xf).reshape(-1, 64), sel=(probe_build.REDUCE_PRIMS['min'],))
    assert np.array_equal(got.view(F).reshape(-1, 16), np.repeat(xf.min(1, keepdims=True), 16, 1))
    # the sum, in the order the four steps add: x = x[source(N)] + x for N = 8, 4, 2, 1, in float32
    xs = (rng.randn(16, 64) * 10.0 ** rng.uniform(-3, 3, (16, 64))).astype(F)
    want = xs.copy()
    for N in (8, 4, 2, 1):
        want = (want[:, source(N)] + want).astype(F)
    got, = device.call('c_row_allreduce', bits(xs), sel=(probe_build.REDUCE_PRIMS['add'],))
    assert np.array_equal(got, bits(want))
    exact = xs.astype(np.float64).reshape(16, 4, 16).sum(2)
    scale = np.abs(xs).astype(np.float64).reshape(16, 4, 16).sum(2)
    assert (np.abs(want.reshape(16, 4, 16)[:, :, 0] - exact) <= 4 * 2.0 ** -24 * scale).all()      # four roundings deep


def test_wave_min_max_rdlane_unif(device):
    rng = np.random.RandomState(9)
    x = (rng.randn(40, 64) * 10.0 ** rng.uniform(-10, 10, (40, 1))).astype(F)
    x[:10] = rng.randint(-2, 3, (10, 64))                                          # ties
    x[10] = 4.0
    lanes = rng.randint(0, 64, 40).astype(np.int32)
    lanes[:4] = (0, 63, 15, 16)
    mn, mx, rd, un = device.call('c_wave_minmax', x, lanes)
    assert np.array_equal(bits(mn), bits(np.repeat(x.min(1, keepdims=True), 64, 1)))
    assert np.array_equal(bits(mx), bits(np.repeat(x.max(1, keepdims=True), 64, 1)))
    assert np.array_equal(bits(rd), bits(np.repeat(x[np.arange(40), lanes][:, None], 64, 1)))
    assert np.array_equal(bits(un), bits(np.repeat(x[:, :1], 64, 1)))
