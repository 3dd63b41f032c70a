"""tests/grasp_refine_host.py, the NumPy restatement of rv_grasp_refine (csrc/rv_dev_grasp_refine.h), against
what the step promises: the ranking of rv_cem_refit, elites copied bit for bit, children that are the parent displaced,
rotated and clamped as the formulas say (within the float32 bounds derived in that module's docstring), valid by the
sampler's checks in float64, falling back to the parent where they are not, and draws keyed by the env and the row
alone.  The GPU tests (tests/test_gpu_grasp_refine.py) compare the kernel with this restatement bit for bit on the same
synthetic inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cem_host
import grasp_refine_host as host

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 40, 48
STRIP = 40      # columns STRIP.. are 0: nothing hit
SAMPLER = {'FRICTION_COEF': 1.0, 'DEPTH_GRAD_THRESH': 0.01, 'DEPTH_GRAD_GAUSSIAN_SIGMA': 1.0, 'DOWNSAMPLE_RATE': 1,
           'MAX_REJECTION_SAMPLES': 100, 'CROP': None, 'MIN_DIST_FROM_BOUNDARY': 4, 'MIN_GRASP_DIST': 2.5,
           'ANGLE_DIST_WEIGHT': 5.0, 'DEPTH_SAMPLES_PER_GRASP': 1, 'MIN_DEPTH_OFFSET': 0.015, 'MAX_DEPTH_OFFSET': 0.03,
           'DEPTH_SAMPLE_WINDOW_HEIGHT': 2, 'DEPTH_SAMPLE_WINDOW_WIDTH': 2}
SAMPLER_CROP = dict(SAMPLER, CROP=[2, 3, 38, 46])
SIGMAS = (2.0, 0.2, 0.004)
WORLD_SEED = 0x1234567811


def synth_images(n):
    """[n, H, W]: a plane at 0.70 m (tilted a little, differently per env), a raised 14 x 10 block at 0.65 m, and a zero
    strip on the right"""
    rr, cc = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, H, W), F)
    for i in range(n):
        img = 0.70 + 0.0004 * (i + 1) * rr - 0.0003 * cc
        img[12:26, 18:28] = 0.65 + 0.001 * i
        img[:, STRIP:] = 0.0
        out[i] = img.astype(F)
    return out


def synth_grasps(n, k, seed=3, integer=False):
    """[n, k, 5] parents around the block: centres that pass the checks, half axes of 3 to 7 px at any angle, depths inside
    their clamp range; ``integer``: end points on whole pixels, as the sampler writes them"""
    rng = np.random.RandomState(seed)
    g = np.zeros((n, k, 5), F)
    cx, cy = rng.uniform(12, 30, (n, k)), rng.uniform(9, 30, (n, k))
    L, th = rng.uniform(3, 7, (n, k)), rng.uniform(0, 2 * np.pi, (n, k))
    g[..., 0], g[..., 1] = cx - L * np.cos(th), cy - L * np.sin(th)
    g[..., 2], g[..., 3] = cx + L * np.cos(th), cy + L * np.sin(th)
    if integer:
        g[..., :4] = np.rint(g[..., :4])
    g[..., 4] = rng.uniform(0.672, 0.678, (n, k))
    return g


def synth_scores(n, k, seed=4):
    """[n, k] with ties, both zeros, NaNs and infinities"""
    rng = np.random.RandomState(seed)
    s = np.round(rng.normal(0, 1, (n, k)), 1).astype(F)
    flat = s.reshape(-1)
    special = [np.nan, 0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0]
    for i, v in enumerate(special):
        if 3 * i + 1 < flat.size:
            flat[3 * i + 1] = v
    return s


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_ranking_is_cem_ranks_over_the_candidates():
    k = 12
    s = synth_scores(3, k)
    assert np.isnan(s).any() and (s == 0).sum() >= 2 and np.isinf(s).any()
    assert len(set(s[np.isfinite(s)].tolist())) < np.isfinite(s).sum()      # ties
    for n in range(3):
        for v in (k, 7, 1):
            cand = np.arange(k) < v
            assert np.array_equal(host.rank(s[n], cand), cem_host.cem_rank(s[n:n + 1, :v])[0])
    g = synth_grasps(3, k)
    out, parent, cnt = host.refine(synth_images(3), g, s, 5, SIGMAS, SAMPLER, count=[k, 7, 3], status=[1, 1, 1])
    for n, v in enumerate((k, 7, 3)):
        ep = min(5, v)
        assert np.array_equal(parent[n, :ep], cem_host.cem_rank(s[n:n + 1, :v])[0, :ep])
        # a row past the count is never a parent
        par = np.where(parent[n] < 0, -1 - parent[n], parent[n])
        assert par.max() < v and set(par[ep:].tolist()) <= set(parent[n, :ep].tolist())
    assert cnt.tolist() == [k, k, k]


def test_elites_are_copies_in_rank_order_and_copy_through_cases():
    k = 9
    img, g, s = synth_images(4), synth_grasps(4, k), synth_scores(4, k)
    g[0, 2] = [np.nan, 1, 2, 3, 4]      # (a NaN row can be an elite: it is copied all the same)
    s[0, 2] = 9.0
    # env 0: every row; env 1: V = 2 < E; env 2: status says no grasp; env 3: count 0
    out, parent, cnt = host.refine(img, g, s, 4, SIGMAS, SAMPLER, count=[k, 2, k, 0], status=[1, 1, -2, 1])
    order0 = cem_host.cem_rank(s[:1])[0]
    assert order0[0] == 2
    assert np.array_equal(bits(out[0, :4]), bits(g[0, order0[:4]])) and np.array_equal(parent[0, :4], order0[:4])
    order1 = cem_host.cem_rank(s[1:2, :2])[0]
    assert np.array_equal(bits(out[1, :2]), bits(g[1, order1])) and np.array_equal(parent[1, :2], order1)
    assert set(np.where(parent[1, 2:] < 0, -1 - parent[1, 2:], parent[1, 2:]).tolist()) <= {0, 1}
    # row j >= E' descends from elite (j - E') mod E'
    for j in range(2, k):
        p = parent[1, j]
        assert (p if p >= 0 else -1 - p) == order1[(j - 2) % 2]
    for n in (2, 3):
        assert np.array_equal(bits(out[n]), bits(g[n])) and np.array_equal(parent[n], np.arange(k)) and cnt[n] == 0
    assert cnt[0] == k and cnt[1] == k
    # E = K: a sort, nothing is drawn
    out, parent, cnt = host.refine(img, g, s, k, SIGMAS, SAMPLER)
    for n in range(4):
        order = cem_host.cem_rank(s[n:n + 1])[0]
        assert np.array_equal(bits(out[n]), bits(g[n, order])) and np.array_equal(parent[n], order)


def _children(n=3, k=64, e=5, sigmas=SIGMAS, sampler=SAMPLER, integer=False, iteration=1):
    img, g, s = synth_images(n), synth_grasps(n, k, integer=integer), synth_scores(n, k)
    out, parent, _ = host.refine(img, g, s, e, sigmas, sampler, world_seed=WORLD_SEED, macro_index=2, iteration=iteration, seed=7)
    z = np.stack([host.normals(WORLD_SEED, i, 2, iteration, 7, np.arange(k)) for i in range(n)])
    return img, g, out, parent, z


def test_child_geometry_against_float64():
    img, g, out, parent, z = _children()
    checked = 0
    for n in range(out.shape[0]):
        for j in range(5, out.shape[1]):
            if parent[n, j] < 0:
                continue
            p, c, zz = g[n, parent[n, j]].astype(np.float64), out[n, j].astype(np.float64), z[n, j].astype(np.float64)
            pc, cc = 0.5 * (p[:2] + p[2:4]), 0.5 * (c[:2] + c[2:4])
            pa, ca = 0.5 * (p[2:4] - p[:2]), 0.5 * (c[2:4] - c[:2])
            want = float(F(SIGMAS[0])) * zz[:2]
            assert np.all(np.abs((cc - pc) - want) <= host.CENTER_TOL), (n, j)
            L = np.hypot(*pa)
            assert abs(np.hypot(*ca) - L) <= host.len_tol(L), (n, j)
            delta = float(F(SIGMAS[1]) * z[n, j, 2])      # (the float32 product the kernel forms)
            turned = np.arctan2(pa[0] * ca[1] - pa[1] * ca[0], pa[0] * ca[0] + pa[1] * ca[1])
            assert abs(np.angle(np.exp(1j * (turned - delta)))) <= host.angle_tol(L), (n, j)
            checked += 1
    assert checked > 100


@pytest.mark.parametrize('sampler', [SAMPLER, SAMPLER_CROP], ids=['whole', 'crop'])
def test_accepted_children_are_valid_in_float64(sampler):
    img, g, out, parent, z = _children(sigmas=(5.0, 0.3, 0.02), sampler=sampler)
    r0, c0, r1, c1 = host.crop_of(sampler, H, W)
    lo_off, hi_off = float(F(sampler['MIN_DEPTH_OFFSET'])), float(F(sampler['MAX_DEPTH_OFFSET']))
    accepted = clamped = 0
    for n in range(out.shape[0]):
        for j in range(5, out.shape[1]):
            if parent[n, j] < 0:
                continue
            c = out[n, j]
            assert np.all(np.isfinite(c))
            # the centre of the row as the kernel forms it, then everything in float64
            ux, uy = float(F(0.5) * (c[0] + c[2])), float(F(0.5) * (c[1] + c[3]))
            assert c0 <= ux <= c1 and r0 <= uy <= r1
            assert min(ux - c0, c1 - ux, uy - r0, r1 - uy) >= sampler['MIN_DIST_FROM_BOUNDARY'] - 1e-3
            win = img[n][int(uy - 2):int(uy + 2), int(ux - 2):int(ux + 2)].astype(np.float64)
            assert win.size == 16 and win.min() != 0
            lo, hi = float(F(win.min()) + F(lo_off)), float(F(win.min()) + F(hi_off))
            assert lo <= float(c[4]) <= hi
            clamped += float(c[4]) in (lo, hi)
            accepted += 1
    assert accepted > 50 and clamped > 5


def test_children_aimed_at_the_zero_strip_or_over_the_boundary_fall_back():
    sig = (12.0, 0.2, 0.004)
    img, g, out, parent, z = _children(sigmas=sig)
    strip = over = kept = 0
    for n in range(out.shape[0]):
        order_elite = parent[n, :5]
        for j in range(5, out.shape[1]):
            e = order_elite[(j - 5) % 5]
            p = g[n, e].astype(np.float64)
            aim = 0.5 * (p[:2] + p[2:4]) + float(F(sig[0])) * z[n, j, :2].astype(np.float64)
            # clearly on the strip: the window [x - 2, x + 2) holds a zero column; clearly over: nearer than the margin
            on_strip = STRIP - 2 + 1.01 < aim[0] < W
            is_over = min(aim[0], W - aim[0], aim[1], H - aim[1]) < SAMPLER['MIN_DIST_FROM_BOUNDARY'] - 1e-3
            if on_strip or is_over:
                assert parent[n, j] == -1 - e, (n, j, aim)
                assert np.array_equal(bits(out[n, j]), bits(g[n, e]))
                strip += on_strip; over += is_over
            if parent[n, j] >= 0:
                assert parent[n, j] == e
                kept += 1
    assert strip > 5 and over > 20 and kept > 20


def test_zero_sigmas_return_the_parent_up_to_the_depth_clamp():
    img, g, out, parent, z = _children(sigmas=(0.0, 0.0, 0.0), integer=True)
    for n in range(out.shape[0]):
        assert np.all(parent[n] >= 0)      # no fallback: the parents themselves pass
        for j in range(5, out.shape[1]):
            p = g[n, parent[n, j]]
            assert np.array_equal(bits(out[n, j, :4]), bits(p[:4]))
            ok, cd = host.check_center(img[n], SAMPLER, F(0.5) * (p[0] + p[2]), F(0.5) * (p[1] + p[3]))
            lo, hi = cd + F(SAMPLER['MIN_DEPTH_OFFSET']), cd + F(SAMPLER['MAX_DEPTH_OFFSET'])
            assert ok and out[n, j, 4] == min(max(p[4], lo), hi)
    # a parent depth outside its range is clamped, not refused
    g2 = g.copy(); g2[..., 4] = 0.2
    out2, parent2, _ = host.refine(img, g2, synth_scores(3, 64), 5, (0.0, 0.0, 0.0), SAMPLER)
    assert np.all(parent2 >= 0) and np.all(out2[:, 5:, 4] > 0.6)


def test_a_row_depends_on_the_env_id_and_the_row_not_on_the_batch():
    k = 9
    img, g, s = synth_images(3), synth_grasps(3, k), synth_scores(3, k)
    kw = dict(world_seed=WORLD_SEED, macro_index=3, iteration=2, seed=5)
    out3, par3, _ = host.refine(img, g, s, 2, SIGMAS, SAMPLER, **kw)
    for n in range(3):      # N = 1 with an env_id_offset: the same env
        out1, par1, _ = host.refine(img[n:n + 1], g[n:n + 1], s[n:n + 1], 2, SIGMAS, SAMPLER, env_id_offset=n, **kw)
        assert np.array_equal(bits(out1[0]), bits(out3[n])) and np.array_equal(par1[0], par3[n])
    # K = 5 and K = 9 with E' = 2 and the same two elites: rows 2 .. 4 agree (row j descends from elite (j - 2) mod 2)
    s5 = s[:, :5].copy()
    top = cem_host.cem_rank(s)[:, :2]
    for n in range(3):
        s5[n] = -5.0
        s5[n, 0], s5[n, 1] = 2.0, 1.0
    g5 = np.stack([np.concatenate([g[n, top[n]], g[n, :3]]) for n in range(3)])
    out5, par5, _ = host.refine(img, g5, s5, 2, SIGMAS, SAMPLER, **kw)
    assert np.array_equal(bits(out5[:, 2:5]), bits(out3[:, 2:5]))
    # iteration, macro_index and seed each change the draws
    z = host.normals(WORLD_SEED, 1, 3, 2, 5, np.arange(k))
    for other in (host.normals(WORLD_SEED, 1, 3, 3, 5, np.arange(k)), host.normals(WORLD_SEED, 1, 4, 2, 5, np.arange(k)),
                  host.normals(WORLD_SEED, 1, 3, 2, 6, np.arange(k)), host.normals(WORLD_SEED, 2, 3, 2, 5, np.arange(k)),
                  host.normals(WORLD_SEED + 1, 1, 3, 2, 5, np.arange(k))):
        assert not np.any(z == other)
    for name, change in (('iteration', dict(iteration=3)), ('macro_index', dict(macro_index=4)), ('seed', dict(seed=6))):
        o, _, _ = host.refine(img, g, s, 2, SIGMAS, SAMPLER, **dict(kw, **change))
        assert not np.array_equal(bits(o[:, 2:]), bits(out3[:, 2:])), name
        assert np.array_equal(bits(o[:, :2]), bits(out3[:, :2])), name


def test_no_two_rows_share_a_philox_block_and_the_key_space_is_its_own():
    words, count = set(), 0
    for gid in (0, 1, 7):
        for macro_index in (0, 1, (1 << 24) - 1):
            for seed in (0, 5):
                for iteration in (0, 1, (1 << 26) - 1):
                    c0, c1, c2, c3 = host.counter_words(macro_index, iteration, seed, gid, np.arange(64))
                    assert np.all(c3 >> np.uint64(24) == host.RV_STREAM_GRASP_REFINE) and np.all(c0 < (1 << 32))
                    for w in zip(c0.tolist(), c1.tolist(), c2.tolist(), c3.tolist()):
                        words.add(w); count += 1
    assert len(words) == count
    # c3 is no other draw's: the bare stream ids 1 .. 7 (reset, random, heuristic, camera, point cloud), and
    # (id << 24) | index of the sampler (5), the push proposals (6), the CEM planner (8), the depth noise (9), the routes (10)
    import antipodal_host
    assert host.RV_STREAM_GRASP_REFINE not in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
    assert (antipodal_host.RV_STREAM_GRASP, cem_host.RV_STREAM_CEM) == (5, 8)
    assert (host.RV_STREAM_GRASP_REFINE << 24) > 10 << 24 | 0xffffff and host.RV_STREAM_GRASP_REFINE < 256
    # the fields of c0 do not overlap
    c0 = int(host.counter_words(0, (1 << 26) - 1, 0, 0, np.array([63]))[0][0])
    assert (c0 >> 6, c0 & 63) == ((1 << 26) - 1, 63)
    with pytest.raises(AssertionError):
        host.counter_words(1 << 24, 0, 0, 0, np.arange(4))
    with pytest.raises(AssertionError):
        host.counter_words(0, 1 << 26, 0, 0, np.arange(4))


def test_displacement_moments_over_4096_children():
    """one parent in the middle of a flat image, sigma 3 px: every child is accepted, and over 4096 of them the mean and
    the variance of the displacement lie within 4 standard errors of (0, sigma^2), per axis"""
    img = np.full((1, 200, 200), 0.7, F)
    g = np.tile(np.array([95.0, 100.0, 105.0, 100.0, 0.72], F), (1, 64, 1))
    s = np.zeros((1, 64), F)
    sigma, d = 3.0, []
    for it in range(66):
        out, parent, _ = host.refine(img, g, s, 1, (sigma, 0.1, 0.001), SAMPLER, world_seed=9, iteration=it)
        assert np.all(parent[0] == 0)
        c = out[0, 1:].astype(np.float64)
        d.append(0.5 * (c[:, :2] + c[:, 2:4]) - np.array([100.0, 100.0]))
    d = np.concatenate(d)[:4096]
    n = len(d)
    assert n == 4096
    for axis in range(2):
        assert abs(d[:, axis].mean()) <= 4 * sigma / np.sqrt(n)
        assert abs(d[:, axis].var() - sigma ** 2) <= 4 * sigma ** 2 * np.sqrt(2.0 / (n - 1))
    assert abs(np.mean(d[:, 0] * d[:, 1])) <= 4 * sigma ** 2 / np.sqrt(n)


def test_struct_size_matches_the_c_layout(tmp_path):
    from robovat_amd import abi
    src = tmp_path / 't.c'
    src.write_text('#include <stdio.h>\n#include "rovat.h"\nint main(){printf("%zu\\n", sizeof(rv_grasp_refine_params));return 0;}\n')
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 't')], check=True)
    out = subprocess.run([str(tmp_path / 't')], capture_output=True, text=True, check=True).stdout.split()
    assert int(out[0]) == C.sizeof(abi.rv_grasp_refine_params) == 48
    names = [n for n, _ in abi.rv_grasp_refine_params._fields_]
    assert names == ['height', 'width', 'macro_index', 'iteration', 'seed', 'n_elites', 'sigma_center', 'sigma_angle',
                     'sigma_depth', 'reserved']
