"""Env states as data on the MI355X: rv_state_save / rv_state_load / rv_branch / rv_plan_simulate against the float C
oracle, bit for bit.  The oracle has no state copy: it runs every trajectory straight through from its reset, so a
restored or branched HIP env is compared with an oracle env that simply took the same actions in a row.  Worlds are
tiny (3 envs, seed 5, auto_reset off); the oracle trajectories are computed once per module and only read."""
import numpy as np
import pytest

from robovat_amd import abi, configs, scenes

pytestmark = pytest.mark.gpu
N, SEED = 3, 5
S, H = 4, 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _push_cfg(n=N, **over):
    scene, names = scenes.make_scene()
    return configs.make_rv_config(env_cfg=configs.push_env_config(**over), n_envs=n, seed=SEED, shape_names=names), scene


def _world(cfg, scene):
    from robovat_amd import lib
    return lib.World(cfg, scene, device=0)


KEYS = ('body', 'joint', 'counters', 'reward', 'done', 'returns')


def _hip_state(w):
    r, d = w.reward()
    return {'body': w.body_state().cpu().numpy(), 'joint': w.joint_state().cpu().numpy(), 'counters': w.env_counters().cpu().numpy(),
            'reward': r.cpu().numpy(), 'done': d.cpu().numpy(), 'returns': w.episode_returns().cpu().numpy()}


def _orc_state(ref):
    r, d = ref.reward()
    return {'body': ref.body_state().astype(np.float32), 'joint': ref.joint_state().astype(np.float32), 'counters': ref.env_counters(),
            'reward': r.astype(np.float32), 'done': d, 'returns': ref.episode_returns().astype(np.float32)}


def _assert_state(got, want, rows=slice(None), what=''):
    for k in KEYS:
        assert _same(got[k][rows], want[k][rows]), (what, k)


def _take(w, k):
    w.set_actions(w.policy_random(k)); w.step_macro()


def _bytes(w):
    return w.save_state().blocks.cpu().numpy()


@pytest.fixture(scope='module')
def oracle():
    """straight-through oracle trajectories: 'a' after reset and after macro indices 0, 1, 2, 3; 'b' after 0, 1, 7, 8;
    'branch'[s]: index 0, then the two action sets of candidate s -- observed xy, reward, done after each, [N, S, H, ...]"""
    from oracle import orc
    cfg, scene = _push_cfg()
    out = {'cfg': cfg, 'scene': scene}

    def run(indices):
        ref = orc.OracleWorld(cfg, scene, double=False)
        ref.reset()
        states = [_orc_state(ref)]
        for k in indices:
            ref.set_actions(ref.policy_random(k)); ref.step_macro()
            states.append(_orc_state(ref))
        return states
    out['a'] = run((0, 1, 2, 3))
    out['b'] = run((0, 1, 7, 8))
    probe = orc.OracleWorld(cfg, scene, double=False)
    actions = np.zeros((N, S, H, probe.G, 4), np.float32)
    for s in range(S):
        for t in range(H):
            actions[:, s, t] = probe.policy_random(10 + s * H + t)
    states = np.zeros((N, S, H, abi.RV_MAXB, 2), np.float32)
    rewards, dones = np.zeros((N, S, H), np.float32), np.zeros((N, S, H), np.uint8)
    for s in range(S):
        ref = orc.OracleWorld(cfg, scene, double=False)
        ref.reset()
        ref.set_actions(ref.policy_random(0)); ref.step_macro()
        for t in range(H):
            ref.set_actions(actions[:, s, t]); ref.step_macro()
            states[:, s, t] = ref.observe()[0].astype(np.float32)[:, :, :2]
            r, d = ref.reward()
            rewards[:, s, t], dones[:, s, t] = r.astype(np.float32), d
    out.update(actions=actions, states=states, rewards=rewards, dones=dones)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_restore_undoes(oracle):
    w = _world(oracle['cfg'], oracle['scene'])
    try:
        w.reset()
        _take(w, 0); _take(w, 1)
        snap = w.save_state()
        assert snap.blocks.shape == (N, w.state_bytes()) and snap.blocks.dtype == w.torch.uint8
        _take(w, 7); _take(w, 8)
        _assert_state(_hip_state(w), oracle['b'][4], what='diverged')
        assert not _same(_hip_state(w)['body'], oracle['a'][2]['body'])
        w.load_state(snap)
        _assert_state(_hip_state(w), oracle['a'][2], what='restored')
        for k in (2, 3):
            _take(w, k)
            _assert_state(_hip_state(w), oracle['a'][k + 1], what='index %d after the restore' % k)
    finally:
        w.close()


def test_restore_per_env(oracle):
    w = _world(oracle['cfg'], oracle['scene'])
    try:
        w.reset()
        _take(w, 0); _take(w, 1)
        snap = w.save_state()
        _take(w, 7); _take(w, 8)
        w.load_state(snap, index=[-1, 1, -1])
        got = _hip_state(w)
        _assert_state(got, oracle['a'][2], rows=slice(1, 2), what='env 1 restored')
        _assert_state(got, oracle['b'][4], rows=[0, 2], what='envs 0 and 2 kept')
        # a device index, and a block that goes to another env: env 0 takes block 2, env 2 stays
        w.load_state(snap, index=w.torch.tensor([2, -1, -1], device=w.device))
        got = _hip_state(w)
        assert _same(got['body'][0], oracle['a'][2]['body'][2]) and _same(got['body'][2], oracle['b'][4]['body'][2])
    finally:
        w.close()


def _poll_to_completion(w):
    done = np.zeros(N, bool)
    for _ in range(10000):
        done |= w.step_poll(max_substeps=50).cpu().numpy().astype(bool)
        if done.all():
            return
    raise AssertionError('the step did not finish')


def test_mid_step(oracle):
    w = _world(oracle['cfg'], oracle['scene'])
    try:
        w.reset()
        w.step_begin(w.policy_random(0))
        assert not w.step_poll(max_substeps=50).cpu().numpy().any()      # (an env.step() is thousands of substeps)
        snap = w.save_state()
        _poll_to_completion(w)
        first = _hip_state(w)
        w.load_state(snap)
        assert not _same(_hip_state(w)['counters'], first['counters'])      # (back in the middle of the step)
        _poll_to_completion(w)
        second = _hip_state(w)
        _assert_state(second, first, what='the two completions')
        # counters 7..9 (substeps / awake substeps / narrow-phase pairs of the LAST LAUNCH) are figures of a launch, not of
        # the env: a poll of 50 substeps reports its own.  Everything else equals the oracle's one-launch step_macro
        want = dict(oracle['a'][1], counters=oracle['a'][1]['counters'].copy())
        want['counters'][:, 7:] = first['counters'][:, 7:]
        _assert_state(first, want, what='step_macro on the oracle')
    finally:
        w.close()


def test_grasp_world():
    from robovat_amd import lib
    from oracle import orc
    env_cfg = configs.grasp_env_config()
    scene, names = scenes.make_scene(env_cfg=env_cfg)
    cfg = configs.make_rv_config(env_cfg=env_cfg, n_envs=N, seed=SEED, shape_names=names)
    w, ref = lib.World(cfg, scene, device=0), orc.OracleWorld(cfg, scene, double=False)
    try:
        w.reset(); ref.reset()
        snap = w.save_state()
        a = ref.policy_random(0)
        a[:, 0, :2] = ref.body_state()[:, 0, :2]      # (aimed at the object)
        ref.set_actions(a); ref.step_macro()
        want = _orc_state(ref)
        w.set_actions(a); w.step_macro()
        _assert_state(_hip_state(w), want, what='first')
        w.load_state(snap)
        assert not _same(_hip_state(w)['joint'], want['joint'])
        w.set_actions(a); w.step_macro()
        _assert_state(_hip_state(w), want, what='again after the restore')
    finally:
        w.close()


def _branch_case(oracle, src, plan):
    import torch
    src.reset()
    _take(src, 0)
    _assert_state(_hip_state(src), oracle['a'][1], what='source before')
    actions = torch.zeros((N, S, H, src.G, 4), dtype=torch.float32, device=src.device)
    for s in range(S):
        for t in range(H):
            actions[:, s, t] = src.policy_random(10 + s * H + t)
    assert _same(actions.cpu().numpy(), oracle['actions'])
    before = _bytes(src)
    states, rewards, dones = plan.plan_simulate(src, actions)
    assert _same(states.cpu().numpy(), oracle['states'])
    assert _same(rewards.cpu().numpy(), oracle['rewards'])
    assert _same(dones.cpu().numpy(), oracle['dones'])
    assert float(np.abs(oracle['states'][:, 1:] - oracle['states'][:, :1]).max()) > 1e-3      # (the candidates differ)
    assert _same(_bytes(src), before)
    _take(src, 1)
    _assert_state(_hip_state(src), oracle['a'][2], what='source after')
    # rv_branch alone: env j of the plan world is env j // S of the source, word for word
    plan.branch_from(src, S)
    assert _same(_bytes(plan), np.repeat(_bytes(src), S, axis=0))


def test_branch(oracle):
    cfg, scene = oracle['cfg'], oracle['scene']
    pcfg, _ = _push_cfg(N * S)
    src, plan = _world(cfg, scene), _world(pcfg, scene)
    try:
        _branch_case(oracle, src, plan)
    finally:
        src.close(); plan.close()


def test_branch_across_the_two_builds_of_the_env_kernel(oracle, monkeypatch):
    cfg, scene = oracle['cfg'], oracle['scene']
    pcfg, _ = _push_cfg(N * S)
    monkeypatch.setenv('RV_ENV_OCC', '1')
    src = _world(cfg, scene)
    monkeypatch.setenv('RV_ENV_OCC', '2')
    plan = _world(pcfg, scene)
    try:
        assert src.env_kernel_build() == abi.RV_ENV_BUILD_OCC1 and plan.env_kernel_build() == abi.RV_ENV_BUILD_OCC2
        _branch_case(oracle, src, plan)
    finally:
        src.close(); plan.close()


def test_branch_with_the_worlds_on_two_streams(oracle):
    """the copy waits for the source's stream and the source's stream for the copy: nobody synchronises in between"""
    import torch
    cfg, scene = oracle['cfg'], oracle['scene']
    pcfg, _ = _push_cfg(N * S)
    src = _world(cfg, scene)
    side = torch.cuda.Stream(device=src.device)
    with torch.cuda.stream(side):
        plan = _world(pcfg, scene)
    try:
        actions = torch.as_tensor(oracle['actions'].copy(), device=src.device)
        torch.cuda.synchronize(src.device)              # (the caller orders its own buffer)
        src.reset()
        _take(src, 0)                                   # (still running on the source's stream when the copy is asked for)
        with torch.cuda.stream(side):
            states, rewards, dones = plan.plan_simulate(src, actions)
        _take(src, 1)                                   # (changes the blocks: must come after the copy)
        side.synchronize()
        assert _same(states.cpu().numpy(), oracle['states']) and _same(rewards.cpu().numpy(), oracle['rewards'])
        _assert_state(_hip_state(src), oracle['a'][2], what='source')
    finally:
        src.close(); plan.close()


def test_errors_change_no_env(oracle):
    import torch
    from robovat_amd import lib
    cfg, scene = oracle['cfg'], oracle['scene']
    src = _world(cfg, scene)
    plan = _world(_push_cfg(N * S)[0], scene)
    other_task = _world(_push_cfg(N * S, TASK_NAME='crossing', LAYOUT_ID=0)[0], scene)
    wrong_size = _world(_push_cfg(N * S + 1)[0], scene)
    genv = configs.grasp_env_config()
    gscene, gnames = scenes.make_scene(env_cfg=genv)
    gsrc = lib.World(configs.make_rv_config(env_cfg=genv, n_envs=N, seed=SEED, shape_names=gnames), gscene, device=0)
    gplan = lib.World(configs.make_rv_config(env_cfg=genv, n_envs=N * S, seed=SEED, shape_names=gnames), gscene, device=0)
    worlds = (src, plan, other_task, wrong_size, gsrc, gplan)
    try:
        for w in worlds:
            w.reset(); w.set_actions(w.policy_random(0)); w.step_sub(20)
        snap = src.save_state()
        before = [_bytes(w) for w in worlds]
        actions = torch.zeros((N, S, H, src.G, 4), dtype=torch.float32, device=src.device)
        with pytest.raises(ValueError):
            other_task.branch_from(src, S)
        with pytest.raises(ValueError):
            wrong_size.branch_from(src, S)
        with pytest.raises(ValueError):
            plan.branch_from(src, S + 1)
        with pytest.raises(ValueError):
            plan.branch_from(src, 0)
        with pytest.raises(ValueError):
            src.branch_from(src, 1)
        with pytest.raises(ValueError):
            gplan.branch_from(src, S)      # (another scene and config)
        foreign = lib.Snapshot(snap.blocks, '0' * 64, snap.config_key)
        with pytest.raises(ValueError):
            src.load_state(foreign)
        with pytest.raises(ValueError):
            src.load_state(snap, index=[0, 5, 1])
        with pytest.raises(ValueError):
            src.load_state(snap, index=[0, -2, 1])
        with pytest.raises(ValueError):
            plan.load_state(snap)                      # (3 blocks, 12 envs, no index)
        with pytest.raises(ValueError):
            other_task.load_state(snap, index=[0] * (N * S))      # (another config)
        with pytest.raises(ValueError):
            gplan.plan_simulate(gsrc, torch.zeros((N, S, H, gsrc.G, 4), device=src.device))
        with pytest.raises(ValueError):
            wrong_size.plan_simulate(src, actions)
        with pytest.raises(ValueError):
            plan.plan_simulate(src, actions[:, :, :0])      # (h = 0)
        # the C entry points themselves: an index outside the buffer leaves the env alone, NULL buffers are refused
        idx = torch.tensor([7, -3, 2 ** 31 - 1], dtype=torch.int32, device=src.device)
        lib.check(src.lib.rv_state_load(src.h, src._ptr(snap.blocks), N, src._ptr(idx)))
        with pytest.raises(ValueError):
            lib.check(src.lib.rv_state_load(src.h, src._ptr(snap.blocks), N - 1, None))
        with pytest.raises(ValueError):
            lib.check(src.lib.rv_state_save(src.h, None))
        with pytest.raises(ValueError):
            lib.check(src.lib.rv_plan_simulate(plan.h, src.h, None, S, H, None, None, None))
        for w, b in zip(worlds, before):
            assert _same(_bytes(w), b)
        # (and the good calls still go through)
        gplan.branch_from(gsrc, S)
        assert _same(_bytes(gplan), np.repeat(_bytes(gsrc), S, axis=0))
        plan.load_state(snap, index=[0, 0, 1, 1, 2, 2] + [-1] * 6)
        assert _same(_bytes(plan)[:6], np.repeat(before[0], 2, axis=0)) and _same(_bytes(plan)[6:], before[1][6:])
    finally:
        for w in worlds:
            w.close()


def test_env_api(oracle):
    """VecPushEnv.save_state / restore_state(mask) / simulate_plans and the same on a PushEnv"""
    import torch
    from robovat_amd.envs.push.push_env import PushEnv, VecPushEnv
    env = VecPushEnv(N, seed=SEED)
    try:
        env.reset()
        env.step(env.sample_random_actions())
        _assert_state(_hip_state(env.world), oracle['a'][1], what='the env is the oracle world')
        snap = env.save_state()
        states, rewards, dones = env.simulate_plans(torch.as_tensor(oracle['actions'].copy()))
        assert dones.dtype == torch.bool and _same(states.cpu().numpy(), oracle['states']) and _same(rewards.cpu().numpy(), oracle['rewards'])
        assert env._plan_world(S) is env._plan_world(S) and env._plan_world(S).n == N * S
        env.step(env.sample_random_actions())
        _assert_state(_hip_state(env.world), oracle['a'][2], what='after planning')
        after = _bytes(env.world)
        env.restore_state(snap, mask=[False, True, False])
        got = _bytes(env.world)
        assert _same(got[1], snap.blocks.cpu().numpy()[1]) and _same(got[[0, 2]], after[[0, 2]])
        env.restore_state(snap)
        assert _same(_bytes(env.world), snap.blocks.cpu().numpy())
        env.step(env.sample_random_actions())      # (the macro index came back with the snapshot)
        _assert_state(_hip_state(env.world), oracle['a'][2], what='after the restore')
    finally:
        env.close()
    one = PushEnv(seed=SEED)
    try:
        one.reset()
        snap = one.save_state()
        a = one._vec.sample_random_actions()[0].cpu().numpy()
        plans = np.stack([np.stack([a, a]), np.stack([-a, a])])      # [2, 2] + action shape
        states, rewards, dones = one.simulate_plans(plans)
        assert states.shape == (2, 2, abi.RV_MAXB, 2) and rewards.shape == (2, 2) and dones.shape == (2, 2)
        obs, r, done, _ = one.step(a)
        assert _same(states[0, 0].cpu().numpy(), obs['position'][:, :2]) and float(rewards[0, 0]) == r
        one.restore_state(snap)
        obs2, r2, done2, _ = one.step(a)
        assert _same(obs2['position'], obs['position']) and r2 == r and done2 == done
    finally:
        one.close()
