"""Every header of robovat_amd/csrc compiles on its own: a translation unit of one line, `#include "<header>"`, passes
the device compiler's syntax check, and the headers of the env program (rv_dev_env.h and every csrc header it includes,
directly or through another) pass the host compiler's too, as the lane emulator of tests/emu compiles
them (-DRV_EMULATE).  A header that reaches for a name it does not include fails here, whatever order rv_kernels.hip
includes it in."""
import os
import re
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'robovat_amd', 'csrc')
HEADERS = sorted(n for n in os.listdir(CSRC) if n.endswith('.h'))


def _includes(header):
    with open(os.path.join(CSRC, header)) as f:
        return re.findall(r'^#include "(rv_\w+\.h)"', f.read(), re.M)


def _env_headers():
    """rv_dev_env.h and the csrc headers it includes, directly or not, in the order they are first met"""
    seen, todo = [], ['rv_dev_env.h']
    while todo:
        h = todo.pop(0)
        if h not in seen:
            seen.append(h)
            todo += _includes(h)
    return seen


ENV_HEADERS = _env_headers()

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
DEVICE = [HIPCC, '-std=c++17', '--offload-arch=gfx950', '--cuda-device-only', '-fsyntax-only', '-x', 'hip']
HOST = ['g++', '-std=c++17', '-DRV_EMULATE', '-fsyntax-only']


def _compile_alone(cmd, header, suffix, tmp_path):
    tu = tmp_path / ('only_' + header[:-2] + suffix)
    tu.write_text('#include "%s"\n' % os.path.join(CSRC, header))
    r = subprocess.run(cmd + [str(tu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, '%s does not compile on its own:\n%s' % (header, r.stdout[-4000:])


def test_env_include_list():
    """the include list was read down to the math header, and no header fell out of it: a csrc header is part of the env
    program, or is built on top of it (it includes rv_dev_env.h), or is one of the three that need neither"""
    assert set(_includes('rv_dev_env.h')) <= set(ENV_HEADERS) <= set(HEADERS)
    assert {'rv_dev_env.h', 'rv_dev_env_types.h', 'rv_dev_wave.h', 'rv_dev_collide.h', 'rv_dev_math.h'} <= set(ENV_HEADERS)
    apart = ('rv_dev_cem.h', 'rv_dev_depth_noise.h', 'rv_dev_state.h')
    assert [h for h in HEADERS if h not in ENV_HEADERS and 'rv_dev_env.h' not in _includes(h)] == list(apart)


@pytest.mark.parametrize('header', HEADERS)
def test_header_alone_device(header, tmp_path):
    _compile_alone(DEVICE, header, '.hip', tmp_path)


@pytest.mark.parametrize('header', ENV_HEADERS)
def test_header_alone_host(header, tmp_path):
    _compile_alone(HOST, header, '.cpp', tmp_path)
