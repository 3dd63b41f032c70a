"""Every lane-emulator test once more, with the env program arranged as the two-waves-per-SIMD build of the env kernel
(k_env_occ2, rv_kernels_occ2.hip) runs it: compiled with RV_SEGMENTS_NOINLINE, all 16 segments of env_program
(rv_dev_env.h) go through the out-of-line seg_* wrappers, each of which rebuilds its Consts with lds_consts(scene, 0),
reaches the env through the file-scope g_shared and forwards its own argument list (gid, zero_counters, count_step,
the body index i, nb).

The tests are those of tests/test_emu_parity.py and the emulator tests of tests/test_gpu_narrow_phase_pairs.py and
tests/test_static_body.py, imported unchanged; only the `emu` fixture differs (tests/emu/librv_emu_seg.so, built on demand like librv_emu.so).

On the host RV_DEV_NOINLINE is `static`, so this leg checks what the wrappers forward and rebuild -- not registers,
scratch, or LDS shared between workgroups, which only the GPU leg (tests/test_gpu_env_builds.py) sees.  A wrapper that
forwards a wrong value (seg_reset_begin handing on gid + 1, say) fails here and passes in tests/test_emu_parity.py.
"""
import pytest

from test_emu_parity import *  # noqa: F401,F403  (the tests)
from test_emu_parity import emu_library
from test_gpu_narrow_phase_pairs import test_emulated_flat_pair_list_with_more_than_four_pairs_per_owner  # noqa: F401
from test_static_body import test_emulated_kernel_with_a_wall_is_bit_exact_vs_float_oracle  # noqa: F401


@pytest.fixture(scope='module')
def emu():  # noqa: F811
    """The lane emulator compiled with RV_SEGMENTS_NOINLINE.  On the host RV_DEV_NOINLINE is `static`: this arrangement
    checks what the seg_* wrappers forward and rebuild, not registers or scratch."""
    return emu_library('seg')
