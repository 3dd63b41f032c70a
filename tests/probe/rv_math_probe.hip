// rv_math_probe.hip -- the scalar primitives of robovat_amd/csrc/rv_dev_math.h, one batch function each (TEST
// INFRASTRUCTURE ONLY; tests/test_math_primitives.py, tests/test_gpu_math_primitives.py).
//
// This one file is compiled twice:
//   * by hipcc for gfx950 with exactly robovat_amd.lib.HIPCC_FLAGS: one trivial kernel per primitive, one thread per
//     element, pointers are DEVICE pointers, launched on the null stream and synchronised before the call returns;
//   * by g++ -x c++ -DRV_EMULATE with the lane emulator's flags: the same bodies in a loop on the CPU, host pointers.
// oracle/orc_math.h goes through the same exports in tests/probe/orc_math_probe.c.
//
// Every export has one signature: int f(int n, int k, const void* a, const void* b, const void* c, void* o) -- n
// elements, up to three input arrays and one output array (rows of floats unless stated), k = draws per element of
// the rng_* functions.  Returns 0, or the hipError_t of the launch / synchronise.
#include "../../robovat_amd/csrc/rv_dev_math.h"

#ifndef RV_PROBE_HASH
#define RV_PROBE_HASH "unknown"
#endif
// sha256 of rv_dev_math.h and this file as they were when the library was compiled (tests/probe/build.py)
extern "C" const char* probe_source_hash() { return RV_PROBE_HASH; }
extern "C" int probe_on_device() { return RV_ON_DEVICE; }

using namespace rv;

#define PROBE_ARGS                                                                                  \
  const float* a = (const float*)a_; const float* b = (const float*)b_; const float* c = (const float*)c_; \
  float* o = (float*)o_;                                                                            \
  const uint32_t* ua = (const uint32_t*)a_; const uint32_t* ub = (const uint32_t*)b_;              \
  const int32_t* ib = (const int32_t*)b_; uint32_t* uo = (uint32_t*)o_; int32_t* io = (int32_t*)o_; \
  (void)a; (void)b; (void)c; (void)o; (void)ua; (void)ub; (void)ib; (void)uo; (void)io; (void)k;

#if RV_ON_DEVICE
#define PROBE(name, ...)                                                                                            \
  __global__ void k_##name(int n, int k, const void* a_, const void* b_, const void* c_, void* o_) {                \
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                                                 \
    if (i >= (size_t)n) return;                                                                                     \
    PROBE_ARGS                                                                                                      \
    __VA_ARGS__                                                                                                     \
  }                                                                                                                 \
  extern "C" int name(int n, int k, const void* a_, const void* b_, const void* c_, void* o_) {                     \
    if (n <= 0) return 0;                                                                                           \
    hipLaunchKernelGGL(k_##name, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, k, a_, b_, c_, o_);        \
    hipError_t err = hipGetLastError();                                                                             \
    if (err == hipSuccess) err = hipDeviceSynchronize();                                                            \
    return (int)err;                                                                                                \
  }
#else
#define PROBE(name, ...)                                                                                            \
  extern "C" int name(int n, int k, const void* a_, const void* b_, const void* c_, void* o_) {                     \
    PROBE_ARGS                                                                                                      \
    for (size_t i = 0; i < (size_t)n; ++i) { __VA_ARGS__ }                                                          \
    return 0;                                                                                                       \
  }
#endif

// ---- scalars
PROBE(p_fsqrtr, o[i] = fsqrtr(a[i]);)
PROBE(p_frintr, o[i] = frintr(a[i]);)
PROBE(p_ffloorr, o[i] = ffloorr(a[i]);)
PROBE(p_fclamp_pm, o[i] = fclamp_pm(a[i], b[i]);)
PROBE(p_fclampr_pm, o[i] = fclampr(a[i], -b[i], b[i]);)
PROBE(p_fdiv, o[i] = a[i] / b[i];)
PROBE(p_frcp, o[i] = 1.0f / a[i];)
PROBE(p_fma, o[i] = rv_fma(a[i], b[i], c[i]);)
// ---- transcendentals
PROBE(p_sincosr, float s, cs; sincosr(a[i], &s, &cs); o[2 * i] = s; o[2 * i + 1] = cs;)
PROBE(p_atan_pos, o[i] = atan_pos(a[i]);)
PROBE(p_atan2r, o[i] = atan2r(a[i], b[i]);)
// ---- quaternions (xyzw rows) and matrices (row-major rows of 9)
PROBE(p_qmul, stq(o + 4 * i, qmul(ldq(a + 4 * i), ldq(b + 4 * i)));)
PROBE(p_qnormalize, stq(o + 4 * i, qnormalize(ldq(a + 4 * i)));)
PROBE(p_qrotv, st3(o + 3 * i, qrotv(ldq(a + 4 * i), ld3(b + 3 * i)));)
PROBE(p_qmat, stm(o + 9 * i, qmat(ldq(a + 4 * i)));)
PROBE(p_qaxis_z, st3(o + 3 * i, qaxis_z(ldq(a + 4 * i)));)
PROBE(p_mulv, st3(o + 3 * i, mulv(ldm(a + 9 * i), ld3(b + 3 * i)));)
PROBE(p_tmulv, st3(o + 3 * i, tmulv(ldm(a + 9 * i), ld3(b + 3 * i)));)
PROBE(p_mulv_mem, st3(o + 3 * i, mulv(a + 9 * i, ld3(b + 3 * i)));)
PROBE(p_tmulv_mem, st3(o + 3 * i, tmulv(a + 9 * i, ld3(b + 3 * i)));)
PROBE(p_euler_to_quat, stq(o + 4 * i, euler_to_quat(a[3 * i], a[3 * i + 1], a[3 * i + 2]));)
PROBE(p_quat_to_euler, float e[3]; quat_to_euler(ldq(a + 4 * i), e); o[3 * i] = e[0]; o[3 * i + 1] = e[1]; o[3 * i + 2] = e[2];)
PROBE(p_quat_yaw, o[i] = quat_yaw(ldq(a + 4 * i));)
// ---- Philox4x32-10: a = counters [n][4] u32, b = keys [n][2] u32, o = [n][4] u32
PROBE(p_philox, philox(ua[4 * i], ua[4 * i + 1], ua[4 * i + 2], ua[4 * i + 3], ub[2 * i], ub[2 * i + 1],
                       uo + 4 * i, uo + 4 * i + 1, uo + 4 * i + 2, uo + 4 * i + 3);)
// ---- streams of k draws from rng_init(seed_lo, seed_hi, gid, stream, arg): a = [n][5] u32, o = [n][k]
#define PROBE_RNG Rng g = rng_init(ua[5 * i], ua[5 * i + 1], ua[5 * i + 2], ua[5 * i + 3], ua[5 * i + 4]);
PROBE(p_rng_uniform01, PROBE_RNG for (int j = 0; j < k; ++j) o[i * k + j] = rng_uniform01(g);)
// b = lo [n], c = hi [n]
PROBE(p_rng_uniform, PROBE_RNG for (int j = 0; j < k; ++j) o[i * k + j] = rng_uniform(g, b[i], c[i]);)
// b = n of randint [n] i32 (> 0), o = [n][k] i32
PROBE(p_rng_randint, PROBE_RNG for (int j = 0; j < k; ++j) io[i * k + j] = rng_randint(g, ib[i]);)
