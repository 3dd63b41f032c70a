"""rv_get_contact_points on the MI355X: field-by-field parity with the NumPy restatement on the oracle's state, the
force balance and friction pyramid of the records, the old hit test as "count > 0", the capacity and the query, and
the HipPhysics contact API."""
import ctypes as C

import numpy as np
import pytest

import contact_host as host
from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu
T, ARM = abi.RV_CP_TABLE, abi.RV_CP_ARM


def _worlds(env_cfg, n, seed, n_ref=64):
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    world = lib.World(configs.make_rv_config(env_cfg=env_cfg, n_envs=n, seed=seed, shape_names=names), scene, device=0)
    rcfg = configs.make_rv_config(env_cfg=env_cfg, n_envs=n_ref, seed=seed, shape_names=names)
    ref = orc.OracleWorld(rcfg, scene, double=False)
    return world, ref, rcfg, scene


def _pad_box(links, arm, f=8, drop=0.02):
    col = list(arm.col_frame).index(f)
    return links[:, f, :3] + np.einsum('nij,j->ni', np.stack([host.qmat(q) for q in links[:, f, 3:7]]),
                                       np.array(list(arm.col_center[col]))) - [0.0, 0.0, drop]


def _compare(world, ref, rcfg, scene, query=(-1, -1, -1, -1)):
    ids, data, count = [t.cpu().numpy() for t in world.contact_points(*query)]
    n_arm = 0
    for env in range(ref.n):
        recs, k = host.records(ref, scene, rcfg, env, query)
        assert count[env] == k, (env, count[env], k)
        for r, (hid, hd, alts) in enumerate(recs):
            if alts is not None:      # (an arm point: the device knows its collider, the oracle leaves a choice)
                link = int(max(ids[env, r, 2], ids[env, r, 3]))
                assert link in alts, (env, r, ids[env, r], sorted(alts))
                hid, hd = alts[link]
            assert np.array_equal(ids[env, r], hid), (env, r, ids[env, r], hid)
            d = data[env, r]
            assert np.allclose(d[0:6], hd[0:6], atol=1e-5, equal_nan=True), (env, r, d[0:6], hd[0:6])
            assert np.allclose(d[6:10], hd[6:10], atol=1e-5, equal_nan=True)
            assert np.allclose(d[12:15], hd[12:15], atol=1e-5) and np.allclose(d[16:19], hd[16:19], atol=1e-5)
            for j in (10, 11, 15):
                assert abs(d[j] - hd[j]) <= 1e-4 * max(abs(hd[j]), 1.0), (env, r, j, d[j], hd[j])
            n_arm += int(ARM in (hid[0], hid[1]) and max(hid[2], hid[3]) >= 0)
    return int(count[:ref.n].sum()), n_arm


def test_records_match_the_restatement_config1_slice():
    """1024 push envs, a 64-env slice: after a macro step, then after a box is dropped into the left finger pad of
    every env and one substep has run (arm records on link 8 with large impulses)."""
    world, ref, rcfg, scene = _worlds(configs.push_env_config(), 1024, 7)
    world.reset(); ref.reset()
    acts = world.policy_random(0)
    world.set_actions(acts); ref.set_actions(acts.cpu().numpy()[:64])
    world.step_macro(); ref.step_macro()
    assert np.array_equal(world.body_state().cpu().numpy()[:64], ref.body_state().astype(np.float32))
    total, _ = _compare(world, ref, rcfg, scene)
    assert total > 64
    _compare(world, ref, rcfg, scene, (0, -1, -1, -1))
    # a box in the finger pad of every env (slot 3), one substep
    p = world.body_params().cpu().numpy(); s = world.body_state().cpu().numpy()
    pad = _pad_box(world.link_poses().cpu().numpy(), scene.arm, drop=0.035 + 0.03 - 0.002)      # (2 mm into the pad's tip)
    p[:, 3] = [1, 0, 1.0, 0.1, 0.5, 0, 0.0, 0]; p[:, 3, 6] = p[:, 0, 6]; s[:, 3] = 0; s[:, 3, 6] = 1; s[:, 3, :3] = pad
    world.set_body_params(p); world.set_body_state(s)
    ref.set_body_params(p[:64].astype(np.float64)); ref.set_body_state(s[:64].astype(np.float64))
    world.step_sub(1); ref.step_sub(1)
    total, n_arm = _compare(world, ref, rcfg, scene)
    assert n_arm >= 64, n_arm
    _compare(world, ref, rcfg, scene, (3, -1, ARM, -1))
    # a link filter keeps exactly the records of that link (the oracle cannot tell every link apart: device only)
    ids, _, count = [t.cpu().numpy() for t in world.contact_points(3, -1, ARM, -1)]
    for f in (8, 9):
        _, _, cf = world.contact_points(3, -1, ARM, f)
        want = [int((ids[e, :min(count[e], abi.RV_CP_MAX), 3] == f).sum()) for e in range(world.n)]
        assert np.array_equal(cf.cpu().numpy(), want), f
    world.close()


def test_records_match_the_restatement_config4_slice():
    """2048 grasp envs, a 64-env slice, after one macro step (the gripper has closed and lifted)."""
    env_cfg = configs.grasp_env_config()
    world, ref, rcfg, scene = _worlds(env_cfg, 2048, 21)
    world.reset(); ref.reset()
    acts = world.policy_random(0)
    world.set_actions(acts); ref.set_actions(acts.cpu().numpy()[:64])
    world.step_macro(); ref.step_macro()
    assert np.array_equal(world.body_state().cpu().numpy()[:64], ref.body_state().astype(np.float32))
    _compare(world, ref, rcfg, scene)
    _compare(world, ref, rcfg, scene, (ARM, -1, -1, -1))
    # a held object: records on both finger-tip links
    ids, data, count = [t.cpu().numpy() for t in world.contact_points(ARM, -1, 0, -1)]
    both = [e for e in range(world.n) if {8, 9} <= set(ids[e, :min(count[e], abi.RV_CP_MAX), 2].tolist())]
    zs = world.body_state().cpu().numpy()[:, 0, 2]
    held = [e for e in both if zs[e] > float(rcfg.table_z) + 0.1]
    print('grasp envs with records on both fingers: %d, of them lifted: %d' % (len(both), len(held)))
    assert held
    world.close()


def _kinetic_world(n=1):
    from robovat_amd import lib
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(n_envs=n, seed=1, shape_names=names)
    return lib.World(cfg, scene, device=0), cfg


def test_resting_box_awake_and_asleep():
    world, cfg = _kinetic_world()
    m = 0.3
    p = np.zeros((1, abi.RV_MAXB, 8), np.float32); s = np.zeros((1, abi.RV_MAXB, 13), np.float32); s[..., 6] = 1
    p[0, 0] = [1, 0, 1.0, m, 0.5, 0, 0.0, 0]; s[0, 0, :3] = (0.6, 0.0, 0.031)
    world.set_body_params(p); world.set_body_state(s)
    mg = m * -float(cfg.gravity_z)
    for n_sub in (150, 3000):          # settling, then long asleep (the impulses of its last solve)
        world.step_sub(n_sub)
        ids, data, count = [t.cpu().numpy() for t in world.contact_points(0, -1, T, -1)]
        assert count[0] == 4
        fn = data[0, :4, 10].sum()
        assert abs(fn - mg) < 0.02 * mg, (n_sub, fn, mg)
        f = world.contact_forces(0, -1, T, -1).cpu().numpy()[0]
        assert np.abs(f - [0.0, 0.0, mg]).max() < 0.02 * mg, f
    assert np.abs(world.body_state().cpu().numpy()[0, 0, 7:13]).max() < 1e-5      # it has come to rest
    world.close()


def test_friction_pyramid_and_old_hit_rule_config1():
    """1024 push envs (with a wall) over three macro steps: every record obeys Bullet's friction pyramid, and for every
    pair of entities count > 0 is the hit test built from query_contacts() and manifold_counts()."""
    from robovat_amd import lib
    env_cfg = configs.push_env_config(**{'SIM.WALL.USE': True, 'SIM.WALL.POSE': [[0.66, 0.0, 0.4], [0, 0, 0]],
                                         'MAX_MOVABLE_BODIES': 3, 'MIN_MOVABLE_BODIES': 3})
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    cfg = configs.make_rv_config(env_cfg=env_cfg, n_envs=1024, seed=3, shape_names=names)
    world = lib.World(cfg, scene, device=0)
    world.reset()
    codes = list(range(abi.RV_MAXB)) + [T, ARM]
    n_checked = n_over = 0
    for step in range(3):
        world.set_actions(world.policy_random(step)); world.step_macro()
        flags = world.query_contacts().cpu().numpy(); counts = world.manifold_counts().cpu().numpy()
        for i, a in enumerate(codes):
            for b in codes[i + 1:]:
                for qa, qb in ((a, b), (b, a)):
                    _, _, count = world.contact_points(qa, -1, qb, -1, capacity=1)
                    got = count.cpu().numpy() > 0
                    want = np.array([host.old_hit(flags[e], counts[e], qa, qb) for e in range(world.n)])
                    assert np.array_equal(got, want), (step, qa, qb, np.nonzero(got != want)[0][:8])
        ids, data, count = [t.cpu().numpy() for t in world.contact_points()]
        par = world.body_params().cpu().numpy()
        for e in range(world.n):
            for r in range(min(count[e], abi.RV_CP_MAX)):
                A, B, _, _ = ids[e, r]
                if A == ARM:
                    continue                                      # (the arm-table record: no forces)
                muB = {T: max(float(cfg.table_friction), float(cfg.ground_friction)), ARM: float(cfg.arm_friction)}.get(int(B))
                mu = par[e, A, 4] * (par[e, B, 4] if muB is None else muB)
                fn, f1, f2 = data[e, r, 10], data[e, r, 11], data[e, r, 15]
                assert fn >= 0.0
                lim = mu * fn
                # (each friction row is clamped to mu x the normal impulse of its own sweep; the stored triple can sit a
                # little outside where a later sweep changed ln, or where mu is not the one assumed here)
                n_over += int(abs(f1) > lim * (1 + 1e-5) + 1e-6 or abs(f2) > lim * (1 + 1e-5) + 1e-6)
                n_checked += 1
    print('friction pyramid: %d records, %d beyond mu fn by more than 1e-5' % (n_checked, n_over))
    assert n_checked > 1000 and n_over <= 0.05 * n_checked
    world.close()


def test_capacity_query_and_errors():
    from robovat_amd import lib
    world, cfg = _kinetic_world(n=4)
    world.reset()
    _, _, full = world.contact_points()
    full = full.cpu().numpy()
    assert full.max() >= 2
    ids = world.torch.full((4, abi.RV_CP_MAX, 4), -7, dtype=world.torch.int32, device=world.device)
    data = world.torch.full((4, abi.RV_CP_MAX, abi.RV_CP_NF), 7.0, dtype=world.torch.float32, device=world.device)
    cnt = world.torch.zeros((4,), dtype=world.torch.int32, device=world.device)
    q = abi.rv_contact_query(-1, -1, -1, -1)
    # capacity 1 into the rows of capacity 1: the true total, one record per env
    lib.check(world.lib.rv_get_contact_points(world.h, C.byref(q), 1, world._ptr(ids), world._ptr(data), world._ptr(cnt)))
    i1, d1, c1 = ids.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(c1, full)
    flat_i = i1.reshape(-1, 4); flat_d = d1.reshape(-1, abi.RV_CP_NF)
    written = np.nonzero((flat_i != -7).any(axis=1))[0]
    assert np.array_equal(written, np.nonzero(full > 0)[0])     # row e of a capacity-1 buffer, for every env with a record
    assert (flat_d[len(full):] == 7.0).all()
    # the query: body 0 against the table from both sides
    a_ids, a_data, a_cnt = [t.cpu().numpy() for t in world.contact_points(0, -1, T, -1)]
    b_ids, b_data, b_cnt = [t.cpu().numpy() for t in world.contact_points(T, -1, 0, -1)]
    assert np.array_equal(a_cnt, b_cnt) and a_cnt.max() > 0
    for e in range(4):
        k = a_cnt[e]
        assert (a_ids[e, :k] == [0, T, -1, -1]).all() and (b_ids[e, :k] == [T, 0, -1, -1]).all()
        assert np.array_equal(b_data[e, :k, 0:3], a_data[e, :k, 3:6]) and np.array_equal(b_data[e, :k, 3:6], a_data[e, :k, 0:3])
        for j in (slice(6, 9), slice(12, 15), slice(16, 19)):
            assert np.array_equal(b_data[e, :k, j], -a_data[e, :k, j])
        assert np.array_equal(b_data[e, :k, 9:12], a_data[e, :k, 9:12]) and np.array_equal(b_data[e, :k, 15], a_data[e, :k, 15])
    for bad in (dict(capacity=0), dict(capacity=abi.RV_CP_MAX + 1), dict(body_a=ARM + 1), dict(body_b=-2),
                dict(body_a=0, link_a=8), dict(link_b=3), dict(body_a=ARM, link_a=abi.RV_NFRAME)):
        with pytest.raises(ValueError):
            world.contact_points(**bad)
    world.close()


def test_hip_physics_contact_api_honours_the_arm_link():
    from robovat_amd.simulation import Simulator
    from robovat_amd.simulation.physics import hip_physics
    sim = Simulator(physics_backend='HipPhysics', worker_id=3)
    sim.reset(); sim.start()
    sim.add_body('sim/table/table.urdf', [[0.6, 0, 0.0], [0, 0, 0]], is_static=True, name='table')
    arm = sim.add_body('sawyer.urdf', is_static=True, is_controllable=True, name='sawyer_arm')
    sim.step()
    phys = sim.physics
    links = phys.world.link_poses().cpu().numpy()[:1]
    pad = _pad_box(links, phys.scene.arm)[0]
    box = sim.add_body('box.urdf', [list(pad), [0, 0, 0]], scale=1.0, name='movable_0')
    sim.step()
    A = hip_physics.ARM_UID
    left = phys.get_contact_point_records((A, 8), box.uid)
    assert left and all(len(r) == 14 for r in left)
    assert all(r[0] == 0 and r[1] == A and r[2] == box.uid and r[3] == 8 and r[4] == -1 for r in left)
    assert len(phys.get_contact_points((A, 8), box.uid)) == len(left)
    assert phys.get_contact_points((A, 9), box.uid) == []
    assert len(phys.get_contact_points(A, box.uid)) == len(left)
    assert sim.check_contact(arm, box) and sim.check_contact(box, arm)
    back = phys.get_contact_point_records(box.uid, (A, 8))
    assert [r[3:5] for r in back] == [(-1, 8)] * len(left) and all(r[1] == box.uid and r[2] == A for r in back)
    assert np.allclose([r[7] for r in back], [tuple(-np.array(r[7])) for r in left])
    assert all(len(cp) == 3 for cp in phys.get_contact_points((A, 8), box.uid))       # cp[-1]: lateralFrictionDir2
