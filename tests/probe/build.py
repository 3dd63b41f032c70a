"""Builds and loads the probes (tests/probe): the primitives of robovat_amd/csrc/rv_dev_math.h and of oracle/orc_math.h
behind one set of batch functions, and the narrow phase of rv_dev_collide.h with the cross-lane primitives of
rv_dev_wave.h behind another.  TEST INFRASTRUCTURE ONLY.

Six libraries, all next to this file:

* ``librv_math_probe_hip.so``   rv_math_probe.hip for gfx950 with exactly ``robovat_amd.lib.HIPCC_FLAGS``.  Only
  ``__graft_entry__.build()`` compiles it (``build_device``); the GPU test loads it and refuses a stale one.
* ``librv_math_probe_host.so``  the same file as host C++ (``-DRV_EMULATE``, the lane emulator's flags).
* ``liborc_math_probe_f32.so`` / ``_f64.so``  orc_math_probe.c with the oracle's flags, float and ``-DORC_DOUBLE``.
* ``librv_collide_probe_hip.so`` / ``_host.so``  rv_collide_probe.hip, built the same two ways (CollideProbe below).

The host libraries are compiled when they are missing or older than their sources.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEV_HEADER = os.path.join(ROOT, 'robovat_amd', 'csrc', 'rv_dev_math.h')
ORC_HEADER = os.path.join(ROOT, 'oracle', 'orc_math.h')
DEV_SRC = os.path.join(HERE, 'rv_math_probe.hip')
ORC_SRC = os.path.join(HERE, 'orc_math_probe.c')
DEVICE_LIB = os.path.join(HERE, 'librv_math_probe_hip.so')
HOST_LIB = os.path.join(HERE, 'librv_math_probe_host.so')
# the collision / wave probe (rv_dev_collide.h over rv_dev_wave.h over rv_dev_math.h): libraries of its own
CSRC = os.path.join(ROOT, 'robovat_amd', 'csrc')
COLLIDE_HEADERS = tuple(os.path.join(CSRC, h) for h in ('rv_dev_math.h', 'rv_dev_wave.h', 'rv_dev_collide.h'))
COLLIDE_SRC = os.path.join(HERE, 'rv_collide_probe.hip')
COLLIDE_DEVICE_LIB = os.path.join(HERE, 'librv_collide_probe_hip.so')
COLLIDE_HOST_LIB = os.path.join(HERE, 'librv_collide_probe_host.so')
ORC_LIBS = {False: os.path.join(HERE, 'liborc_math_probe_f32.so'), True: os.path.join(HERE, 'liborc_math_probe_f64.so')}

# the lane emulator's flags (tests/test_emu_parity.py EMU_FLAGS) without OpenMP: the loops here are serial
HOST_FLAGS = ['-O2', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mfma', '-shared']
# the oracle's flags (oracle/Makefile) without OpenMP
ORC_FLAGS = ['-O2', '-std=gnu11', '-fPIC', '-ffp-contract=off', '-mfma', '-fno-fast-math', '-Wall', '-Wno-unused-function', '-shared']

# name -> (rows of the inputs, row of the output); a row is (kind, width): 'f' real, 'u' uint32, 'i' int32, and a
# width of 'k' means k draws per element.  The order is the order of the a, b, c arguments.
F1, F2, F3, F4, F9 = ('f', 1), ('f', 2), ('f', 3), ('f', 4), ('f', 9)
FUNCS = {
    'p_fsqrtr': ((F1,), F1), 'p_frintr': ((F1,), F1), 'p_ffloorr': ((F1,), F1),
    'p_fclamp_pm': ((F1, F1), F1), 'p_fclampr_pm': ((F1, F1), F1),
    'p_fdiv': ((F1, F1), F1), 'p_frcp': ((F1,), F1), 'p_fma': ((F1, F1, F1), F1),
    'p_sincosr': ((F1,), F2), 'p_atan_pos': ((F1,), F1), 'p_atan2r': ((F1, F1), F1),
    'p_qmul': ((F4, F4), F4), 'p_qnormalize': ((F4,), F4), 'p_qrotv': ((F4, F3), F3), 'p_qmat': ((F4,), F9),
    'p_qaxis_z': ((F4,), F3), 'p_mulv': ((F9, F3), F3), 'p_tmulv': ((F9, F3), F3),
    'p_mulv_mem': ((F9, F3), F3), 'p_tmulv_mem': ((F9, F3), F3),
    'p_euler_to_quat': ((F3,), F4), 'p_quat_to_euler': ((F4,), F3), 'p_quat_yaw': ((F4,), F1),
    'p_philox': ((('u', 4), ('u', 2)), ('u', 4)),
    'p_rng_uniform01': ((('u', 5),), ('f', 'k')),
    'p_rng_uniform': ((('u', 5), F1, F1), ('f', 'k')),
    'p_rng_randint': ((('u', 5), ('i', 1)), ('i', 'k')),
}


def probe_source_hash():
    """sha256 over rv_dev_math.h and rv_math_probe.hip: baked into the device probe when it is compiled."""
    h = hashlib.sha256()
    for path in (DEV_HEADER, DEV_SRC):
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def collide_source_hash():
    """sha256 over rv_dev_math.h, rv_dev_wave.h, rv_dev_collide.h and rv_collide_probe.hip, baked into the device build."""
    h = hashlib.sha256()
    for path in COLLIDE_HEADERS + (COLLIDE_SRC,):
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _compile(cmd, out):
    """Compile to a private name and rename: a concurrent reader never sees a half-written library."""
    tmp = '%s.%d.tmp' % (out, os.getpid())
    try:
        subprocess.run(cmd + ['-o', tmp], check=True)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def build_device(verbose=False):
    """Cross-compile the device probe like librovat_hip.so: robovat_amd.lib.HIPCC_FLAGS, imported and not restated."""
    from robovat_amd import lib
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + list(lib.HIPCC_FLAGS) + ['-DRV_PROBE_HASH="%s"' % probe_source_hash(), DEV_SRC]
    if verbose:
        print(' '.join(cmd))
    _compile(cmd, DEVICE_LIB)
    return DEVICE_LIB


def build_host(force=False):
    if force or _stale(HOST_LIB, (DEV_HEADER, DEV_SRC)):
        _compile(['g++', '-DRV_EMULATE'] + HOST_FLAGS + ['-x', 'c++', DEV_SRC], HOST_LIB)
    return HOST_LIB


def build_collide_device(verbose=False):
    """The collision / wave probe for gfx950, with the product's flags like build_device."""
    from robovat_amd import lib
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc] + list(lib.HIPCC_FLAGS) + ['-DRV_PROBE_HASH="%s"' % collide_source_hash(), COLLIDE_SRC]
    if verbose:
        print(' '.join(cmd))
    _compile(cmd, COLLIDE_DEVICE_LIB)
    return COLLIDE_DEVICE_LIB


def build_collide_host(force=False):
    if force or _stale(COLLIDE_HOST_LIB, COLLIDE_HEADERS + (COLLIDE_SRC,)):
        _compile(['g++', '-DRV_EMULATE'] + HOST_FLAGS + ['-x', 'c++', COLLIDE_SRC], COLLIDE_HOST_LIB)
    return COLLIDE_HOST_LIB


def build_oracle(double, force=False):
    out = ORC_LIBS[bool(double)]
    if force or _stale(out, (ORC_HEADER, ORC_SRC)):
        _compile(['gcc'] + ORC_FLAGS + (['-DORC_DOUBLE'] if double else []) + [ORC_SRC, '-lm'], out)
    return out


def build_all(verbose=False):
    build_device(verbose=verbose)
    build_host(force=True)
    build_oracle(False, force=True)
    build_oracle(True, force=True)
    build_collide_device(verbose=verbose)
    build_collide_host(force=True)


def _bind(path):
    lib = C.CDLL(path)
    for name in FUNCS:
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


_NP = {'u': np.uint32, 'i': np.int32}


class HostProbe(object):
    """One of the CPU libraries.  ``call(name, *inputs, k=1)`` takes numpy arrays (anything that converts to the
    library's types: ``real`` is float32, or float64 for the ORC_DOUBLE build) and returns a new array [n, width]
    (width 1 is squeezed to [n])."""

    def __init__(self, path, real=np.float32):
        self.lib, self.real, self.path = _bind(path), real, path

    def _dtype(self, kind):
        return self.real if kind == 'f' else _NP[kind]

    def call(self, name, *inputs, **kw):
        k = int(kw.get('k', 1))
        ins, (okind, owidth) = FUNCS[name]
        assert len(inputs) == len(ins), name
        arrs = []
        n = None
        for x, (kind, width) in zip(inputs, ins):
            x = np.ascontiguousarray(np.asarray(x).astype(self._dtype(kind), copy=False)).reshape(-1, width)
            n = x.shape[0] if n is None else n
            assert x.shape[0] == n, (name, x.shape, n)
            arrs.append(x)
        ow = k if owidth == 'k' else owidth
        out = np.zeros((n, ow), self._dtype(okind))
        ptrs = [x.ctypes.data_as(C.c_void_p) for x in arrs] + [None] * (3 - len(arrs))
        status = getattr(self.lib, name)(n, k, ptrs[0], ptrs[1], ptrs[2], out.ctypes.data_as(C.c_void_p))
        assert status == 0, (name, status)
        return out[:, 0] if ow == 1 and owidth != 'k' else out


def host_probe():
    """rv_dev_math.h compiled for the host."""
    p = HostProbe(build_host())
    assert p.lib.probe_on_device() == 0
    return p


def oracle_probe(double=False):
    """orc_math.h, float or double."""
    p = HostProbe(build_oracle(double), np.float64 if double else np.float32)
    assert p.lib.probe_is_double() == int(bool(double))
    return p


class DeviceProbe(object):
    """The gfx950 build: same ``call`` as HostProbe, numpy in and out; the arrays travel through torch tensors on
    the current device, whose pointers the library takes.  A missing or stale library is an error, never a skip."""

    def __init__(self):
        if not os.path.exists(DEVICE_LIB):
            raise RuntimeError('%s is not built: run __graft_entry__.build()' % DEVICE_LIB)
        # torch first, as lib.World does: the probe must bind to the HIP runtime torch has loaded, not bring a second
        # one into the process (which then sees no device, and neither does anything loaded after it)
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError('the device probe needs a GPU')
        torch.cuda.init()
        self.torch = torch
        self.lib = _bind(DEVICE_LIB)
        self.lib.probe_source_hash.restype = C.c_char_p
        built = self.lib.probe_source_hash().decode()
        if built != probe_source_hash():
            raise RuntimeError('%s is stale: built from %s, rv_dev_math.h + rv_math_probe.hip are now %s; run '
                               '__graft_entry__.build()' % (DEVICE_LIB, built, probe_source_hash()))
        assert self.lib.probe_on_device() == 1

    def call(self, name, *inputs, **kw):
        t = self.torch
        k = int(kw.get('k', 1))
        ins, (okind, owidth) = FUNCS[name]
        assert len(inputs) == len(ins), name
        tdt = {'f': t.float32, 'u': t.int32, 'i': t.int32}
        ndt = {'f': np.float32, 'u': np.uint32, 'i': np.int32}
        tens = []
        n = None
        for x, (kind, width) in zip(inputs, ins):
            x = np.ascontiguousarray(np.asarray(x).astype(ndt[kind], copy=False)).reshape(-1, width)
            n = x.shape[0] if n is None else n
            assert x.shape[0] == n, (name, x.shape, n)
            # (uint32 travels as the same bits in an int32 tensor)
            tens.append(t.from_numpy(x.view(np.int32) if kind == 'u' else x).to('cuda'))
        ow = k if owidth == 'k' else owidth
        out = t.zeros((n, ow), dtype=tdt[okind], device='cuda')
        t.cuda.synchronize()
        ptrs = [C.c_void_p(x.data_ptr()) for x in tens] + [None] * (3 - len(tens))
        status = getattr(self.lib, name)(n, k, ptrs[0], ptrs[1], ptrs[2], C.c_void_p(out.data_ptr()))
        if status != 0:
            raise RuntimeError('%s: hipError_t %d' % (name, status))
        res = out.cpu().numpy()
        if okind == 'u':
            res = res.view(np.uint32)
        return res[:, 0] if ow == 1 and owidth != 'k' else res


# ------------------------------------------------------------------------------------------ collision / wave probe --
# The second binding: every export of rv_collide_probe.hip is  int f(int n, <selectors: int ...>, <arrays ...>)  with the
# arrays in the order below, ('in' | 'out', kind, words per item); kinds as above plus 'm', one DevMan as raw words.
# A cross-lane export takes one value per lane: an item is a wave of 64 words.
def _cf(*rows):
    return tuple(rows)


COLLIDE_FUNCS = {
    'c_row_step': (2, _cf(('in', 'u', 64), ('out', 'u', 64))),
    'c_row_allreduce': (1, _cf(('in', 'u', 64), ('out', 'u', 64))),
    'c_wave_minmax': (0, _cf(('in', 'f', 64), ('in', 'i', 1), ('out', 'f', 64), ('out', 'f', 64), ('out', 'f', 64), ('out', 'f', 64))),
    'c_support_v': (0, _cf(('in', 'f', 48), ('in', 'i', 1), ('in', 'f', 3), ('out', 'f', 1), ('out', 'i', 1), ('out', 'f', 3), ('out', 'f', 1))),
    'c_closest_segment': (0, _cf(('in', 'f', 6), ('out', 'f', 2))),
    'c_closest_triangle': (0, _cf(('in', 'f', 9), ('out', 'f', 3))),
    'c_simplex_weights': (0, _cf(('in', 'f', 12), ('in', 'i', 1), ('out', 'f', 4), ('out', 'i', 1))),
    'c_gjk_epa': (0, _cf(('in', 'f', 48), ('in', 'i', 1), ('in', 'f', 48), ('in', 'i', 1), ('in', 'f', 3), ('in', 'f', 1), ('in', 'i', 1),
                         ('in', 'i', 1), ('in', 'i', 8), ('out', 'i', 1), ('out', 'f', 11), ('out', 'i', 8))),
    'c_man_add': (0, _cf(('in', 'm', 0), ('in', 'f', 11), ('in', 'i', 1), ('out', 'm', 0))),
    'c_plane_space': (0, _cf(('in', 'f', 3), ('out', 'f', 6))),
}
ROW_PRIMS = {'row_ror_f': 0, 'row_ror_i': 1, 'row_ror_fmax': 2, 'row_ror_imin': 3, 'row_ror_min': 4, 'row_ror_add': 5,
             'grp_ror_max': 6, 'grp_bcast': 7}
REDUCE_PRIMS = {'fmax': 0, 'imin': 1, 'min': 2, 'add': 3}
NOT_AVAILABLE = -1
GUARD_WORDS = 16
GUARD = 0xA5A5A5A5          # fills the guard words AND the output words before the call: an unwritten word shows
_CNP = {'f': np.float32, 'u': np.uint32, 'i': np.int32, 'm': np.uint32}


def _check_collide_inputs(name, arrs):
    """What the code under test takes on trust (rv_collide_probe.hip, launch contract): refuse it here, before a launch."""
    def within(x, lo, hi):
        assert x.size == 0 or (int(x.min()) >= lo and int(x.max()) <= hi), (name, int(x.min()), int(x.max()), lo, hi)
    if name == 'c_support_v':
        within(arrs[1], 1, 16)
    elif name == 'c_simplex_weights':
        within(arrs[1], 1, 4)
    elif name == 'c_gjk_epa':
        within(arrs[1], 1, 16); within(arrs[3], 1, 16)
        within(arrs[8][:, 0], 0, 3); within(arrs[8][:, 2:], 0, 2 ** 31 - 1)
    elif name == 'c_man_add':
        within(arrs[0][:, 0].view(np.int32), 0, 4)
    elif name == 'c_wave_minmax':
        within(arrs[1], 0, 63)


class CollideProbe(object):
    """rv_collide_probe.hip, host or gfx950 build.  ``call(name, *inputs, sel=())`` takes one numpy array per 'in' row
    ([n, words]) and returns one new array per 'out' row.  The device build takes its pointers from torch tensors on
    the current device; each output lies between GUARD_WORDS guard words on either side, which must come back
    untouched.  A missing or stale device library is an error, never a skip."""

    def __init__(self, device=False):
        self.device = bool(device)
        if self.device:
            if not os.path.exists(COLLIDE_DEVICE_LIB):
                raise RuntimeError('%s is not built: run __graft_entry__.build()' % COLLIDE_DEVICE_LIB)
            import torch          # first, as in DeviceProbe: the probe binds to the HIP runtime torch has loaded
            if not torch.cuda.is_available():
                raise RuntimeError('the device probe needs a GPU')
            torch.cuda.init()
            self.torch = torch
            path = COLLIDE_DEVICE_LIB
        else:
            path = build_collide_host()
        self.path = path
        self.lib = C.CDLL(path)
        self.lib.probe_source_hash.restype = C.c_char_p
        if self.device:
            built = self.lib.probe_source_hash().decode()
            if built != collide_source_hash():
                raise RuntimeError('%s is stale: built from %s, rv_dev_math.h + rv_dev_wave.h + rv_dev_collide.h + '
                                   'rv_collide_probe.hip are now %s; run __graft_entry__.build()' % (path, built, collide_source_hash()))
        assert self.lib.probe_on_device() == int(self.device)
        self.man_words = int(self.lib.probe_devman_words())
        assert self.lib.probe_gjkcache_words() == 8
        for name, (nsel, rows) in COLLIDE_FUNCS.items():
            fn = getattr(self.lib, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_int] * (1 + nsel) + [C.c_void_p] * len(rows)

    def call(self, name, *inputs, **kw):
        sel = tuple(int(s) for s in kw.get('sel', ()))
        nsel, rows = COLLIDE_FUNCS[name]
        assert len(sel) == nsel, (name, sel)
        width = lambda kind, w: self.man_words if kind == 'm' else w       # noqa: E731
        ins = [r for r in rows if r[0] == 'in']
        assert len(inputs) == len(ins), name
        arrs, n = [], None
        for x, (_, kind, w) in zip(inputs, ins):
            x = np.ascontiguousarray(np.asarray(x).astype(_CNP[kind], copy=False)).reshape(-1, width(kind, w))
            n = x.shape[0] if n is None else n
            assert x.shape[0] == n, (name, x.shape, n)
            arrs.append(x)
        _check_collide_inputs(name, arrs)
        outs = [np.full(n * width(kind, w) + 2 * GUARD_WORDS, GUARD, np.uint32) for d, kind, w in rows if d == 'out']
        if self.device:
            t = self.torch
            tin = [t.from_numpy(x.view(np.int32)).to('cuda') for x in arrs]
            tout = [t.from_numpy(o.view(np.int32)).to('cuda') for o in outs]
            t.cuda.synchronize()
            pin = [C.c_void_p(x.data_ptr()) for x in tin]
            pout = [C.c_void_p(o.data_ptr() + 4 * GUARD_WORDS) for o in tout]
        else:
            pin = [x.ctypes.data_as(C.c_void_p) for x in arrs]
            pout = [C.c_void_p(o.ctypes.data + 4 * GUARD_WORDS) for o in outs]
        it_in, it_out = iter(pin), iter(pout)
        ptrs = [next(it_in) if d == 'in' else next(it_out) for d, _, _ in rows]
        status = getattr(self.lib, name)(n, *(sel + tuple(ptrs)))
        if status == NOT_AVAILABLE:
            raise NotImplementedError('%s%s is not available in %s' % (name, sel, self.path))
        if status != 0:
            raise RuntimeError('%s: hipError_t %d' % (name, status))
        if self.device:
            outs = [o.cpu().numpy().view(np.uint32) for o in tout]
        res = []
        for o, (_, kind, w) in zip(outs, [r for r in rows if r[0] == 'out']):
            assert (o[:GUARD_WORDS] == GUARD).all() and (o[-GUARD_WORDS:] == GUARD).all(), '%s wrote outside an output array' % name
            res.append(o[GUARD_WORDS:-GUARD_WORDS].view(_CNP[kind]).reshape(n, width(kind, w)).copy())
        return tuple(res)
