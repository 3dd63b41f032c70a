"""How well the LDS reads of each kernel are batched: compiles ONE translation unit to gfx950 assembly with the
library's own flags and counts, per kernel, instructions, LDS reads, LDS writes and the s_waitcnt that wait on them.

    python tools/lds_wait_report.py [rv_kernels.hip | rv_kernels_occ2.hip] [--csrc DIR] [--asm FILE] [-D...]

--csrc DIR: take the translation unit from another source tree (the parent commit's, for the side-by-side table);
--asm FILE: count an assembly file that exists already.  It only counts -- it is not a test and asserts nothing.
(A wait's lgkmcnt field also covers scalar loads; the env kernels have next to none inside their loops.)"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)


def assemble(src, defines):
    from robovat_amd import lib
    flags = [f for f in lib.HIPCC_FLAGS if f not in ('-shared', '-fPIC')]
    tmp = tempfile.mkdtemp(prefix='lds_wait_')
    out = os.path.join(tmp, os.path.basename(src) + '.s')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc] + flags + ['-DRV_SOURCE_HASH="report"', '--cuda-device-only', '-S'] + defines + [src, '-o', out], check=True)
    return out


def count(asm_path):
    """{function: counts} of every kernel and out-of-line device function of an assembly file (a body runs from its
    label to .Lfunc_end; the two-waves-per-SIMD unit keeps the segments of the env program out of line)"""
    kernels = set(re.findall(r'^\s*\.type\s+([^\s,]+),@function', open(asm_path).read(), re.M))
    rows, cur = {}, None
    for line in open(asm_path):
        m = re.match(r'^([A-Za-z_][\w$.]*):', line)
        if m and m.group(1) in kernels:
            cur = rows.setdefault(m.group(1), dict(insts=0, reads=0, writes=0, w_lgkm=0, w_vm=0, w_all=0))
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
        if cur is None:
            continue
        t = line.strip()
        if not t or t[0] in '.;' or t.endswith(':'):
            continue
        op = t.split()[0]
        cur['insts'] += 1
        if op.startswith('ds_read') or op.startswith('ds_load'):
            cur['reads'] += 1
        elif op.startswith('ds_write') or op.startswith('ds_store'):
            cur['writes'] += 1
        elif op == 's_waitcnt':
            cur['w_all'] += 1
            cur['w_lgkm'] += 'lgkmcnt' in t
            cur['w_vm'] += 'vmcnt' in t
    return rows


def demangle(name):
    import shutil
    tool = shutil.which('c++filt') or shutil.which('llvm-cxxfilt')
    if tool is None:
        return name
    return subprocess.run([tool, name], capture_output=True, text=True).stdout.strip() or name


def main():
    args = sys.argv[1:]
    defines = [a for a in args if a.startswith('-D')]
    args = [a for a in args if not a.startswith('-D')]
    csrc, asm, unit = os.path.join(ROOT, 'robovat_amd', 'csrc'), None, 'rv_kernels.hip'
    while args:
        a = args.pop(0)
        if a == '--csrc':
            csrc = args.pop(0)
        elif a == '--asm':
            asm = args.pop(0)
        else:
            unit = a
    if asm is None:
        asm = assemble(os.path.join(csrc, unit), defines)
    print('# %s' % (asm if '--asm' in sys.argv else os.path.join(os.path.basename(os.path.normpath(csrc)), unit)))
    print('%-44s %8s %7s %7s %8s %8s %8s %10s' % ('kernel', 'insts', 'LDS rd', 'LDS wr', 'waits', 'lgkmcnt', 'vmcnt', 'rd / lgkm'))
    for name, r in sorted(count(asm).items()):
        short = demangle(name)
        print('%-44s %8d %7d %7d %8d %8d %8d %10.2f' % (short[:44], r['insts'], r['reads'], r['writes'], r['w_all'], r['w_lgkm'], r['w_vm'],
                                                         r['reads'] / max(r['w_lgkm'], 1)))
    print('# assembly kept at %s' % asm)


if __name__ == '__main__':
    main()
