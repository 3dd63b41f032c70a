"""Limb dynamics (rv_config.limb_dynamics): while the arm touches an awake body the seven
limb joints are unknowns of the contact solver, with the joint-space inertia of the chain, the contact
Jacobians and one effort-limited POSITION_CONTROL motor row per joint (controllable_body.py:458-466,
bullet_physics.py:1061-1104).  PyBullet is absent, so the anchors are analytic:

  * the joint-space inertia M(q) and the generalised gravity force equal the ones derived from the
    kinetic / potential energy of the eight masses, computed here from finite differences of the
    link frames (an independent route: no composite-body sum)
  * a gripper that comes down ON a box stalls: the box is not pressed into the table, and at rest
    the joint torques that balance the contact force and gravity are within the joint efforts, one of
    them at its limit (the kinematic limb presses with tens of kN)
  * a light push is unchanged: the box still moves with the velocity of the pusher
"""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes
from test_kat_contact import BACKENDS, HIP_BUILDS, _hip_world, close_hip_worlds  # noqa: F401

G = 9.8


def _world(backend, limb=1, n=1):
    scene, names = scenes.make_scene()
    cfg = configs.make_rv_config(env_cfg=configs.push_env_config(**{'PHYSICS.LIMB_DYNAMICS': limb}),
                                 n_envs=n, seed=1, shape_names=names)
    if backend in HIP_BUILDS:
        return _hip_world(backend, cfg, scene), cfg, scene
    from oracle import orc
    return orc.OracleWorld(cfg, scene, double=(backend == 'oracle64')), cfg, scene


def _qmat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _plane_space(n):
    """btPlaneSpace1: the two friction directions of a contact normal."""
    if abs(n[2]) > 0.7071067811865475:
        a = n[1] * n[1] + n[2] * n[2]; k = 1.0 / np.sqrt(a)
        p = np.array([0.0, -n[2] * k, n[1] * k])
        return p, np.array([a * k, -n[0] * p[2], n[0] * p[1]])
    a = n[0] * n[0] + n[1] * n[1]; k = 1.0 / np.sqrt(a)
    p = np.array([-n[1] * k, n[0] * k, 0.0])
    return p, np.array([-n[2] * p[1], n[2] * p[0], a * k])


def _frames(w, q):
    js = w.joint_state(); js[0, :7, 0] = q; js[0, :7, 1] = 0.0
    w.set_joint_state(js)
    lp = w.link_poses()[0]
    return lp[:8, :3].copy(), [_qmat(lp[i, 3:7]) for i in range(8)]


def _energy_matrices(w, scene, q, h=1e-5):
    """M(q) and the generalised gravity force from central differences of the link frames."""
    arm = scene.arm
    m = np.array([arm.link_mass[i] for i in range(8)])
    com = np.array([[arm.link_com[i][k] for k in range(3)] for i in range(8)])
    inert = np.array([[arm.link_inertia[i][k] for k in range(3)] for i in range(8)])
    p0, R0 = _frames(w, q)
    Jv = np.zeros((8, 3, 7)); Jw = np.zeros((8, 3, 7))
    for j in range(7):
        dq = np.zeros(7); dq[j] = h
        pp, Rp = _frames(w, q + dq); pm, Rm = _frames(w, q - dq)
        for i in range(8):
            cp = pp[i] + Rp[i] @ com[i]; cm = pm[i] + Rm[i] @ com[i]
            Jv[i, :, j] = (cp - cm) / (2 * h)
            S = (Rp[i] - Rm[i]) / (2 * h) @ R0[i].T              # [omega]x
            Jw[i, :, j] = [S[2, 1], S[0, 2], S[1, 0]]
    M = np.zeros((7, 7)); g = np.array([0.0, 0.0, -G]); Q = np.zeros(7)
    for i in range(8):
        Iw = R0[i] @ np.diag(inert[i]) @ R0[i].T
        M += m[i] * Jv[i].T @ Jv[i] + Jw[i].T @ Iw @ Jw[i]
        Q += m[i] * (g @ Jv[i])
    return M, Q


def test_joint_space_inertia_and_gravity_match_the_energies():
    w, cfg, scene = _world('oracle64')
    w.reset()
    rng = np.random.RandomState(3)
    lo = np.array([scene.arm.q_lo[j] for j in range(7)]); hi = np.array([scene.arm.q_hi[j] for j in range(7)])
    dt = float(cfg.dt)
    for _ in range(4):
        q = lo + (hi - lo) * (0.2 + 0.6 * rng.rand(7))
        M_ref, Q_ref = _energy_matrices(w, scene, q)
        _frames(w, q)
        M, Mi, blo, bhi = w.limb_debug(0)
        assert np.abs(M - M_ref).max() < 2e-4 * np.abs(M_ref).max(), np.abs(M - M_ref).max()
        assert np.abs(M @ Mi - np.eye(7)).max() < 1e-9
        assert np.all(np.linalg.eigvalsh(M) > 0)
        # motor rows: +- tau dt minus the holding torque (the motor already delivers -Q against gravity);
        # the free motion has spent nothing here (joints at rest)
        tau = np.array([1.0 / scene.arm.inv_tau_max[j] for j in range(7)])
        assert np.allclose(bhi, np.maximum(0.0, tau * dt + Q_ref * dt), rtol=0, atol=2e-4 * tau * dt)
        assert np.allclose(blo, np.minimum(0.0, -tau * dt + Q_ref * dt), rtol=0, atol=2e-4 * tau * dt)


def _press(w, cfg, n_chunks=120):
    """Top-down gripper above a 6 cm box, commanded to a pose whose pads are 3 cm above the table."""
    w.reset()
    tz = float(w.body_params()[0, 0, 6])
    quat = np.array([1.0, 0.0, 0.0, 0.0])
    start = np.concatenate([[0.60, 0.0, tz + 0.30], quat]).astype(np.float32)
    end = np.concatenate([[0.60, 0.0, tz + 0.14 + 0.03], quat]).astype(np.float32)
    js = w.joint_state()
    for _ in range(8):
        q = w.compute_ik(start[None])[0]
        js[0, :7, 0] = q; js[0, :7, 1] = 0.0
        w.set_joint_state(js)
    p = np.zeros((1, abi.RV_MAXB, 8)); p[0, 0] = [1, 0, 1.0, 0.2, 0.5, 0, tz, 0]
    s = np.zeros((1, abi.RV_MAXB, 13)); s[..., 6] = 1; s[0, 0, :3] = [0.60, 0.0, tz + 0.031]
    w.set_body_params(p); w.set_body_state(s)
    w.set_link_target(end[None])
    for _ in range(n_chunks):
        w.step_sub(10)
    return tz


@pytest.mark.parametrize('backend', BACKENDS)
def test_gripper_that_lands_on_a_box_stalls(backend):
    w, cfg, scene = _world(backend, limb=1)
    tz = _press(w, cfg)
    st = w.body_state()[0, 0]
    assert st[2] - tz > 0.031 - 1.5e-3                            # not pressed into the table
    assert np.abs(w.joint_state()[0, :7, 1]).max() < 0.02         # the limb has stalled
    hand_z = w.link_poses()[0, 8, 2] - tz
    assert hand_z > 0.14 + 0.055                                  # ... on top of the box, short of its target
    if backend == 'oracle64':                                     # (finite differences of the frames need doubles)
        # statics.  (a) the motor torques (row impulse / dt plus the holding torque -Q) are within the
        # joint efforts and the joints that limit the push are AT their effort; (b) the arm is at rest, so
        # motor torque + gravity + the contact forces' generalised force vanish: the last is computed here
        # from the manifold impulses and finite-difference Jacobians of the contact points
        dt = float(cfg.dt)
        n, man = w.manifold(0, abi.RV_MAXB + abi.RV_NBB)
        F = man[:n, 10].sum() / dt                                # normal force, box <- pads
        assert 20.0 < F < 600.0, F
        q = w.joint_state()[0, :7, 0].copy()
        st = w.body_state()[0, 0]
        M, Mi, lo, hi = w.limb_debug(0)
        lam = w.last_motor_impulse.copy()
        _, Q = _energy_matrices(w, scene, q)
        tau = np.array([1.0 / scene.arm.inv_tau_max[j] for j in range(7)])
        motor = lam / dt - Q
        assert np.all(np.abs(motor) <= tau * (1 + 1e-4)), motor / tau
        assert np.sum(np.abs(motor) >= tau * (1 - 1e-3)) >= 1, motor / tau
        Rb = _qmat(st[3:7]); C = np.zeros(7); h = 1e-5
        p7, R7 = _frames(w, q); p7, R7 = p7[7], R7[7]
        for i in range(n):
            wa = st[:3] + Rb @ man[i, 0:3]                        # contact point (on the box; the pad is there too)
            nrm = man[i, 6:9]
            t1, t2 = _plane_space(nrm)
            f_arm = -(nrm * man[i, 10] + t1 * man[i, 11] + t2 * man[i, 12]) / dt
            loc = R7.T @ (wa - p7)
            for j in range(7):
                dq = np.zeros(7); dq[j] = h
                pp, Rp = _frames(w, q + dq); pm, Rm = _frames(w, q - dq)
                C[j] += f_arm @ ((pp[7] + Rp[7] @ loc) - (pm[7] + Rm[7] @ loc)) / (2 * h)
        _frames(w, q)
        # (the 50-sweep Gauss-Seidel is not converged with a 100 : 1 mass ratio across the box: the stalled arm
        # jitters at ~1e-3 rad/s and a single substep balances to about a tenth)
        assert np.abs(lam / dt + C).max() < 0.15 * np.abs(C).max(), (lam / dt, C)
    if hasattr(w, 'w'):
        w.close()


@pytest.mark.parametrize('backend', ['oracle64'])
def test_kinematic_limb_crushes_the_same_box(backend):
    """The gap the mode closes: the kinematic limb drives the box into the table."""
    w, cfg, scene = _world(backend, limb=0)
    tz = _press(w, cfg, 60)
    n, man = w.manifold(0, abi.RV_MAXB + abi.RV_NBB)
    assert man[:n, 10].sum() / float(cfg.dt) > 5e3
    assert w.body_state()[0, 0, 2] - tz < 0.031 - 5e-3


@pytest.mark.gpu
def test_limb_dynamics_env_steps_match_the_oracle_bit_for_bit():
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene()
    for ecfg in (configs.push_env_config(**{'PHYSICS.LIMB_DYNAMICS': 1, 'MIN_MOVABLE_BODIES': 1, 'MAX_MOVABLE_BODIES': 4}),
                 configs.grasp_env_config(**{'PHYSICS.LIMB_DYNAMICS': 1})):
        cfg = configs.make_rv_config(env_cfg=ecfg, n_envs=48, seed=5, shape_names=names)
        w, ref = lib.World(cfg, scene, device=0), orc.OracleWorld(cfg, scene, double=False)
        w.reset(); ref.reset()
        w.rollout(4, first_macro_index=0, auto_reset=True, record=False); ref.rollout(4, 0, True)
        assert np.array_equal(w.body_state().cpu().numpy(), ref.body_state().astype(np.float32))
        assert np.array_equal(w.joint_state().cpu().numpy(), ref.joint_state().astype(np.float32))
        ws, rs = w.stats(), ref.stats()
        for k in ('env_steps', 'substeps', 'awake_substeps', 'useful', 'successes'):
            assert ws[k] == rs[k], k
        w.close()


@pytest.mark.gpu
def test_lone_limb_island_stops_on_its_own_while_another_island_sweeps_on():
    """Several awake bodies of which ONE touches the arm and is an island by itself: the limb motor rows belong to that
    island and stop sweeping with it, while the island of another body may need more sweeps.  (Found by
    tools/parity_sweep.py at 256 envs: the oracle kept iterating the motor rows for as long as ANY island iterated;
    env 73 of seed 1001 is such a case in its third env.step().)"""
    from robovat_amd import lib
    from oracle import orc
    scene, names = scenes.make_scene()
    ecfg = configs.push_env_config(**{'PHYSICS.LIMB_DYNAMICS': 1, 'MIN_MOVABLE_BODIES': 1, 'MAX_MOVABLE_BODIES': 4})
    cfg = configs.make_rv_config(env_cfg=ecfg, n_envs=96, seed=1001, shape_names=names)
    w, ref = lib.World(cfg, scene, device=0), orc.OracleWorld(cfg, scene, double=False)
    w.reset(); ref.reset()
    w.rollout(4, first_macro_index=0, auto_reset=True, record=False); ref.rollout(4, 0, True)
    assert np.array_equal(w.body_state().cpu().numpy(), ref.body_state().astype(np.float32))
    assert np.array_equal(w.joint_state().cpu().numpy(), ref.joint_state().astype(np.float32))
    w.close()
