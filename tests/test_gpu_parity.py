"""HIP path vs CPU oracle on identical seeded inputs (runs on the MI355X box).

Tolerances (FP32 path, stated per SURVEY.md §8c):
  * vs the float oracle the kernels are written to match operation for
    operation: body poses must agree to 1e-6 m / 1e-6 (quaternion) after whole
    macro steps (thousands of substeps) and the integer bookkeeping (substep
    counts, phases, flags) must be identical;
  * vs the double oracle (pose-error oracle of record): see
    tests/test_gpu_scale.py::test_pose_error_vs_double_oracle_recorded.
"""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu


def _worlds(n, seed, double=False, **over):
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene()
    env_cfg = configs.push_env_config(**over)
    cfg = configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, shape_names=names)
    return lib.World(cfg, scene, device=0), orc.OracleWorld(cfg, scene, double=double), cfg


def _cmp(world, ref, tol):
    got = world.body_state().cpu().numpy()
    want = ref.body_state().astype(np.float32)
    err = np.abs(got - want).max()
    assert err <= tol, err
    assert np.array_equal(world.env_counters().cpu().numpy(), ref.env_counters())
    assert np.array_equal(world.manifold_counts().cpu().numpy(), ref.manifold_counts())
    jerr = np.abs(world.joint_state().cpu().numpy() - ref.joint_state().astype(np.float32)).max()
    assert jerr <= tol, jerr
    return err


def test_reset_and_macro_steps_match_float_oracle():
    world, ref, cfg = _worlds(16, seed=5)
    world.reset(); ref.reset()
    _cmp(world, ref, 1e-6)
    assert world.stats()['substeps'] == ref.stats()['substeps']
    for k in range(2):
        a = ref.policy_random(k)
        assert np.array_equal(world.policy_random(k).cpu().numpy(), a)
        world.set_actions(a); ref.set_actions(a)
        world.step_macro(); ref.step_macro()
        _cmp(world, ref, 1e-6)
        ws, rs = world.stats(), ref.stats()
        for key in ('substeps', 'env_steps', 'unsafe', 'ineffective', 'useful', 'max_substeps'):
            assert ws[key] == rs[key], key
        r, d = world.reward(); rr, rd = ref.reward()
        assert np.allclose(r.cpu().numpy(), rr, atol=1e-6) and np.array_equal(d.cpu().numpy(), rd)


def test_concave_crossing_layout_matches_float_oracle():
    world, ref, cfg = _worlds(8, seed=21, TASK_NAME='crossing', LAYOUT_ID=0, MOVABLE_NAME='CONCAVE', MAX_STEPS=4)
    world.reset(); ref.reset()
    _cmp(world, ref, 1e-6)
    a = ref.policy_random(0)
    world.set_actions(a); ref.set_actions(a)
    world.step_macro(); ref.step_macro()
    _cmp(world, ref, 1e-6)
    r, d = world.reward(); rr, rd = ref.reward()
    assert np.allclose(r.cpu().numpy(), rr, atol=1e-5) and np.array_equal(d.cpu().numpy(), rd)


def test_free_fall_and_resting_kat_on_gpu():
    """Analytic KATs straight through the C ABI: free fall z(t) and a resting box."""
    from robovat_amd import lib
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(n_envs=4, seed=1, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    p = np.zeros((4, abi.RV_MAXB, 8), np.float32); p[:, 0] = [1, 0, 1.0, 0.2, 0.5, 0, 0.0, 0]
    s = np.zeros((4, abi.RV_MAXB, 13), np.float32); s[..., 6] = 1; s[:, 0, :3] = [0.6, 0.0, 0.5]
    world.set_body_params(p); world.set_body_state(s)
    world.step_sub(100)
    z = world.body_state().cpu().numpy()[:, 0, 2]
    # semi-implicit Euler with per-step damping 0.96**dt
    vz, zz, damp = 0.0, 0.5, float(cfg.lin_damp)
    for _ in range(100):
        vz = (vz - 9.8e-3) * damp; zz += vz * 1e-3
    assert np.allclose(z, zz, atol=1e-5)
    world.step_sub(900)
    st = world.body_state().cpu().numpy()[:, 0]
    assert np.allclose(st[:, 2], 0.031, atol=5e-4)         # half height 0.03 + margin
    assert np.abs(st[:, 7:13]).max() < 1e-3                # at rest
    assert (world.manifold_counts().cpu().numpy()[:, 0] == 4).all()


def test_full_size_properties_config2():
    """BASELINE config 2 size (1024 envs): size-independent properties."""
    world, ref, cfg = _worlds(1024, seed=1234)
    world.reset()
    st = world.body_state().cpu().numpy()
    prm = world.body_params().cpu().numpy()
    assert np.isfinite(st).all()
    assert (prm[..., 0] == 1).all()                        # 4 active bodies everywhere
    q = st[..., 3:7]
    assert np.allclose((q * q).sum(-1), 1.0, atol=1e-5)    # unit quaternions
    assert (st[..., 2] > prm[..., 6] - 1e-3).all()         # nothing below the table after reset
    # pairwise xy distance >= ~MARGIN at placement; after settling still separated
    a = world.policy_random(0)
    world.set_actions(a); world.step_macro()
    s = world.stats()
    assert s['env_steps'] == 1024 and s['substeps'] > 1024 * 1000
    st2 = world.body_state().cpu().numpy()
    assert np.isfinite(st2).all()
    # idempotence: a done-less env stepped with the same RNG stream reproduces itself
    world2 = _worlds(1024, seed=1234)[0]
    world2.reset(); world2.set_actions(a); world2.step_macro()
    assert np.array_equal(world2.body_state().cpu().numpy(), st2)


def test_rollout_matches_oracle_rollout():
    world, ref, cfg = _worlds(12, seed=31, MAX_STEPS=2)
    world.reset(); ref.reset()
    r, d = world.rollout(3, first_macro_index=4, auto_reset=True, record=True)
    ref.rollout(3, 4, True)
    _cmp(world, ref, 1e-6)
    ws, rs = world.stats(), ref.stats()
    assert ws['env_steps'] == rs['env_steps'] == 36 and ws['substeps'] == rs['substeps']
    assert np.isfinite(r.cpu().numpy()).all() and d.cpu().numpy().shape == (3, 12)


def test_async_rollout_is_a_prefix_of_the_lockstep_trajectories():
    """rv_rollout_async: the envs share a pool of env.step() calls.  How many steps
    each env gets depends on timing, but WHAT it computes does not: the oracle run
    with the same per-env step counts must give bit-identical states."""
    world, ref, cfg = _worlds(96, seed=77, MAX_STEPS=3)
    world.reset(); ref.reset()
    total = 96 * 4
    taken = world.rollout_async(total, first_macro_index=2).cpu().numpy()
    # every env that asked while the pool lasted got its step: exactly `total` steps overall
    assert taken.sum() == total and taken.min() >= 1
    ref.rollout_counts(taken, 2)
    _cmp(world, ref, 1e-6)
    ws, rs = world.stats(), ref.stats()
    assert ws['env_steps'] == rs['env_steps'] == total and ws['substeps'] == rs['substeps']


def test_wide_rollout_matches_oracle_bit_for_bit():
    """512 envs x 8 steps in one launch (coasting, lazy kinematics, wake queries with
    distance-bound culling, island solver, register-resident motor runs, resets): every
    body state, joint state, counter and manifold size equals the float oracle's."""
    world, ref, cfg = _worlds(512, seed=2024, MAX_STEPS=5)
    world.reset(); ref.reset()
    world.rollout(8, first_macro_index=0, auto_reset=True, record=False)
    ref.rollout(8, 0, True)
    err = _cmp(world, ref, 0.0)
    assert err == 0.0
    ws, rs = world.stats(), ref.stats()
    for k in ('env_steps', 'substeps', 'awake_substeps', 'max_substeps'):
        assert ws[k] == rs[k], k


@pytest.mark.parametrize('over', [{'PHYSICS.ARM_EFFORT_LIMIT': 1}, {'PHYSICS.GRAVITY_XY': (0.3, -0.2)},
                                  {'PHYSICS.SLEEP_STEPS': 0}, {'PHYSICS.SOLVER_TOL_REST': 1e-7},
                                  {'PHYSICS.SLEEP_STEPS': 0, 'PHYSICS.SOLVER_TOL_REST': 1e-6, 'MIN_MOVABLE_BODIES': 4, 'MAX_MOVABLE_BODIES': 4}])
def test_optional_physics_match_oracle_bit_for_bit(over):
    """The optional pieces -- joint-effort limit on the arm's contact forces, a tilted gravity
    vector (set_gravity), no deactivation at all -- through a rollout with resets."""
    world, ref, cfg = _worlds(48, seed=5, MAX_STEPS=3, **over)
    world.reset(); ref.reset()
    world.rollout(4, first_macro_index=0, auto_reset=True, record=False)
    ref.rollout(4, 0, True)
    assert _cmp(world, ref, 0.0) == 0.0
    ws, rs = world.stats(), ref.stats()
    for k in ('env_steps', 'substeps', 'awake_substeps'):
        assert ws[k] == rs[k], k


def test_partial_batch_trajectories_equal_step_macro():
    """rv_step_begin / rv_step_poll: (a) used in lock step with a substep budget and (b) as a
    work-conserving loop with a time budget, where every env runs at its own pace -- after its
    k-th env.step() each env is in the state the float oracle reaches with step_macro, bit for
    bit, and the observation / reward the poll hands back are those of that step."""
    import torch
    n, K = 48, 3
    world, ref, cfg = _worlds(n, seed=41)
    world.reset(); ref.reset()
    acts = [ref.policy_random(k) for k in range(K)]
    states, rewards = [], []
    for k in range(K):
        ref.set_actions(acts[k]); ref.step_macro()
        states.append(ref.body_state().astype(np.float32)); rewards.append(ref.reward()[0].astype(np.float32))
    # (a) lock step, 700 substeps per launch
    for k in range(K):
        world.step_begin(acts[k])
        left = np.ones(n, bool); polls = 0
        while left.any():
            fin = world.step_poll(max_substeps=700).cpu().numpy().astype(bool)
            assert not (fin & ~left).any()
            left &= ~fin; polls += 1
        assert polls > 3
        assert np.array_equal(world.body_state().cpu().numpy(), states[k])
    # (b) every env at its own pace, 200 us of GPU time per launch, results through the poll buffers
    world2 = _worlds(n, seed=41)[0]
    world2.reset()
    out = world2.poll_buffers(point_cloud=True)
    A = torch.as_tensor(np.stack(acts), device='cuda')                       # [K, N, G, 4]
    cnt = torch.zeros(n, dtype=torch.long, device='cuda')
    world2.step_begin(A[0])
    ar = torch.arange(n, device='cuda')
    seen = np.zeros((K, n), bool); polls = 0
    while int(cnt.min()) < K:
        fin = world2.step_poll(max_usec=200, out=out).bool()
        polls += 1
        assert polls < 20000
        if not bool(fin.any()):
            continue
        idx = fin.nonzero().flatten()
        k_done = cnt[idx]
        got_pos = out['obs']['position'][idx].cpu().numpy(); got_r = out['reward'][idx].cpu().numpy()
        st = world2.body_state()[idx].cpu().numpy()
        for j, (i, kk) in enumerate(zip(idx.cpu().numpy(), k_done.cpu().numpy())):
            assert np.array_equal(st[j], states[kk][i])                         # the state right after its kk-th step
            assert np.array_equal(got_pos[j], states[kk][i][:, :3]) and got_r[j] == rewards[kk][i]
            seen[kk, i] = True
        cnt[idx] += 1
        nxt = fin & (cnt < K)
        if bool(nxt.any()):
            world2.step_begin(A[cnt.clamp(max=K - 1), ar], mask=nxt.to(torch.uint8))
    assert seen.all() and polls > K
    pc = out['obs']['point_cloud'].cpu().numpy()
    assert np.isfinite(pc).all()
    world.close(); world2.close()


def test_partial_batches_with_auto_reset():
    """rv_set_auto_reset: a step begun on an env whose episode is over resets it (what generate_episodes does between
    episodes, episode_generation.py:36-46) and the poll hands back what env.reset() returns.  (a) Round by round with
    unlimited polls the envs are where the float oracle is with step_macro (which skips finished envs) followed by
    reset(mask = finished before the round); (b) with a 300-substep budget per poll, every env at its own pace, each
    env ends in the same state after the same number of calls."""
    import torch
    n, R = 48, 6
    world, ref, cfg = _worlds(n, seed=43, MAX_STEPS=2)
    world.set_auto_reset(True)
    world.reset(); ref.reset()
    out = world.poll_buffers(point_cloud=False)
    acts = [ref.policy_random(k) for k in range(R)]
    resets = 0
    for k in range(R):
        done_before = ref.reward()[1].astype(bool) if k else np.zeros(n, bool)
        ref.set_actions(acts[k]); ref.step_macro()
        if done_before.any():
            ref.reset(mask=done_before.astype(np.uint8)); resets += int(done_before.sum())
        world.step_begin(acts[k])
        fin = world.step_poll(out=out).cpu().numpy().astype(bool)
        assert fin.all()
        assert np.array_equal(world.body_state().cpu().numpy(), ref.body_state().astype(np.float32)), k
        assert np.array_equal(world.joint_state().cpu().numpy(), ref.joint_state().astype(np.float32)), k
        d = out['done'].cpu().numpy().astype(bool); r = out['reward'].cpu().numpy()
        assert not d[done_before].any() and (r[done_before] == 0).all()        # env.reset(): reward 0, not done
        pos = out['obs']['position'].cpu().numpy()
        assert np.array_equal(pos[done_before], ref.observe()[0][done_before].astype(np.float32))
    assert resets >= n                                                          # MAX_STEPS = 2: every env was reset at least once
    final = world.body_state().cpu().numpy()
    # (b) the same R calls per env, cut into 300-substep polls, envs restarted as they finish
    w2 = _worlds(n, seed=43, MAX_STEPS=2)[0]
    w2.set_auto_reset(True); w2.reset()
    A = torch.as_tensor(np.stack(acts), device='cuda')
    cnt = torch.zeros(n, dtype=torch.long, device='cuda'); ar = torch.arange(n, device='cuda')
    w2.step_begin(A[0]); polls = 0
    while int(cnt.min()) < R:
        fin = w2.step_poll(max_substeps=300).bool()
        polls += 1
        assert polls < 5000
        cnt += fin.long()
        go = fin & (cnt < R)
        if bool(go.any()):
            w2.step_begin(A[cnt.clamp(max=R - 1), ar], mask=go.to(torch.uint8))
    assert np.array_equal(w2.body_state().cpu().numpy(), final)
    world.close(); w2.close()


def test_both_builds_of_the_env_kernel_match_the_oracle(monkeypatch):
    """librovat_hip.so holds the env kernel twice (rv_env_kernel.h): the register-rich build for one env per SIMD and
    the two-waves-per-SIMD build a world with more envs than SIMDs launches.  RV_ENV_OCC forces either on a small
    world: both equal the float oracle bit for bit over resets and whole env.step() calls."""
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(MIN_MOVABLE_BODIES=2, MAX_MOVABLE_BODIES=4, MAX_STEPS=3),
                                 n_envs=96, seed=41, shape_names=names)
    ref = orc.OracleWorld(cfg, scene, double=False)
    ref.reset(); ref.rollout(5, 0, True)
    for occ in ('1', '2'):
        monkeypatch.setenv('RV_ENV_OCC', occ)
        w = lib.World(cfg, scene, device=0)
        assert w.env_kernel_build() == int(occ)
        w.reset(); w.rollout(5, first_macro_index=0, auto_reset=True, record=False)
        assert np.array_equal(w.body_state().cpu().numpy(), ref.body_state().astype(np.float32)), occ
        assert np.array_equal(w.joint_state().cpu().numpy(), ref.joint_state().astype(np.float32)), occ
        assert np.array_equal(w.env_counters().cpu().numpy(), ref.env_counters()), occ
        assert np.array_equal(w.manifold_counts().cpu().numpy(), ref.manifold_counts()), occ
        w.close()


def test_concentric_overlaps_run_epa_from_a_grown_simplex():
    """Bodies teleported INTO each other (same centre and orientation: identical shapes give a mirror-symmetric
    difference body, GJK ends with the origin ON a segment / triangle of its simplex).  Until round 5 such a pair was
    reported as 'touching, depth 0'; now the simplex is grown into a tetrahedron and EPA measures the overlap
    (rv_dev_collide.h simplex_expand; closed forms: tests/test_independent_pin.py).  HIP == float oracle through the
    push-out, and the pair manifolds of the identical-shape pairs hold deep points."""
    world, ref, cfg = _worlds(64, seed=5)
    world.reset(); ref.reset()
    st = ref.body_state().copy()
    for a, b in ((0, 1), (2, 3)):
        st[:, b, :7] = st[:, a, :7]
    st[:, :, 2] += 0.03; st[:, :, 7:] = 0
    ref.set_body_state(st); world.set_body_state(st)
    ref.step_sub(1); world.step_sub(1)
    _cmp(world, ref, 0.0)
    same = ref.body_params()[:, 0, 1] == ref.body_params()[:, 1, 1]
    deep = sum(1 for i in range(64) if same[i] and ref.manifold(i, abi.RV_MAXB)[0] > 0 and ref.manifold(i, abi.RV_MAXB)[1][:, 9].min() < -0.005)
    assert same.sum() >= 8 and deep == same.sum(), (deep, same.sum())
    ref.step_sub(60); world.step_sub(60)
    _cmp(world, ref, 0.0)


def test_solver_exits_stay_close_to_plain_sweeps_at_1024_envs():
    """The GPU leg of tests/test_solver_exits.py at BASELINE configs[1]'s size (round-4 review, weak item 9): the shipped
    exits (residual 1e-5 N s, stall 12, <= 50 sweeps) against Bullet's 50 plain sweeps on the MI355X, one env.step() per
    env from the same reset states and actions.  Contact-rich pushes diverge chaotically, so the statement is
    distributional: median / 75th percentile over envs of the worst body, outcome counts within 1.5 % of the env steps."""
    n = 1024
    a, _, _ = _worlds(n, seed=7)
    b, _, _ = _worlds(n, seed=7, **{'PHYSICS.SOLVER_STALL': 0, 'PHYSICS.SOLVER_TOL': 0.0})
    a.reset(); b.reset()
    p0 = a.body_state().cpu().numpy()
    assert np.median(np.abs(p0[..., :3] - b.body_state().cpu().numpy()[..., :3]).max((-1, -2))) < 5e-5     # the same episodes
    b.set_body_params(a.body_params()); b.set_body_state(a.body_state()); a.set_body_state(a.body_state())
    act = a.policy_random(0)
    a.set_actions(act); b.set_actions(act); a.step_macro(); b.step_macro()
    sa, sb = a.body_state().cpu().numpy(), b.body_state().cpu().numpy()
    dev = np.linalg.norm(sa[..., :3] - sb[..., :3], axis=-1).max(-1)
    moved = np.linalg.norm(sa[..., :2] - p0[..., :2], axis=-1).max(-1)
    assert (moved > 1e-3).mean() > 0.15
    assert np.median(dev) < 1.5e-4 and np.percentile(dev, 75) < 1e-3, (np.median(dev), np.percentile(dev, 75))
    ta, tb = a.stats(), b.stats()
    for k in ('useful', 'unsafe', 'ineffective'):
        assert abs(ta[k] - tb[k]) <= 16, (k, ta[k], tb[k])
