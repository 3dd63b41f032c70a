"""The env-state entry points (rv_state_bytes / rv_state_save / rv_state_load / rv_branch / rv_plan_simulate) are
declared in include/rovat.h, bound in robovat_amd/abi.py and listed in lib.SYMBOLS (tests/test_abi.py then checks that
the library exports them); the Python surface on top of them exists.  No GPU."""
import ctypes as C
import os
import re

from robovat_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('rv_state_bytes', 'rv_state_save', 'rv_state_load', 'rv_branch', 'rv_plan_simulate')


def _header():
    with open(os.path.join(ROOT, 'include', 'rovat.h')) as f:
        return re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)


def test_declared_bound_and_listed():
    text = _header()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in abi.STATE_API, name
        assert name in lib.SYMBOLS, name
    assert sorted(abi.STATE_API) == sorted(NAMES)


def test_bindings_match_the_declarations():
    """argument counts and the 64-bit return of rv_state_bytes, read off the header"""
    text = _header()
    for name, (res, args) in abi.STATE_API.items():
        m = re.search(r'(\w+)\s+%s\s*\(([^)]*)\)' % name, text)
        assert m, name
        assert len([a for a in m.group(2).split(',') if a.strip()]) == len(args), name
        assert (res is abi.i64) == (m.group(1) == 'int64_t'), name

    class Fn(object):
        restype = argtypes = None
    handle = type('H', (), {n: Fn() for n in NAMES})()
    abi.bind_state_api(handle)
    assert handle.rv_state_bytes.restype is abi.i64 and handle.rv_branch.argtypes == [C.c_void_p, C.c_void_p, abi.i32]


def test_config_key_ignores_the_two_world_size_fields_only():
    from robovat_amd import configs, scenes
    _, names = scenes.make_scene()
    a = configs.make_rv_config(n_envs=3, seed=5, shape_names=names)
    b = configs.make_rv_config(n_envs=12, seed=5, env_id_offset=40, shape_names=names)
    c = configs.make_rv_config(n_envs=3, seed=6, shape_names=names)
    assert abi.config_key(a) == abi.config_key(b) != abi.config_key(c)
    assert a.n_envs == 3 and b.env_id_offset == 40      # (the configs themselves are not touched)


def test_python_surface():
    from robovat_amd import policies
    from robovat_amd.envs.push.push_env import PushEnv, VecPushEnv
    for name in ('state_bytes', 'save_state', 'load_state', 'branch_from', 'plan_simulate'):
        assert callable(getattr(lib.World, name)), name
    for cls in (VecPushEnv, PushEnv):
        for name in ('save_state', 'restore_state', 'simulate_plans'):
            assert callable(getattr(cls, name)), (cls.__name__, name)
    snap = lib.Snapshot(None, 'h', b'k')
    assert (snap.blocks, snap.source_hash, snap.config_key) == (None, 'h', b'k')
    assert issubclass(policies.ShootingPushPolicy, policies.Policy)
