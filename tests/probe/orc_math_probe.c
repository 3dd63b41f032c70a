/* orc_math_probe.c -- the scalar primitives of oracle/orc_math.h behind the exports of rv_math_probe.hip (TEST
 * INFRASTRUCTURE ONLY).  Built twice: float (must equal the host compile of rv_dev_math.h bit for bit) and
 * -DORC_DOUBLE (libm sin / cos / atan2 and double quaternion algebra: the float64 reference of the accuracy tests).
 * Arrays are rows of `real` (float or double by build) unless stated; see rv_math_probe.hip for the signature. */
#include "../../oracle/orc_math.h"

int probe_is_double(void) { return (int)(sizeof(real) == 8); }

#define PROBE(name, ...)                                                                            \
  int name(int n, int k, const void* a_, const void* b_, const void* c_, void* o_) {                \
    const real* a = (const real*)a_; const real* b = (const real*)b_; const real* c = (const real*)c_; \
    real* o = (real*)o_;                                                                            \
    const uint32_t* ua = (const uint32_t*)a_; const uint32_t* ub = (const uint32_t*)b_;            \
    const int32_t* ib = (const int32_t*)b_; uint32_t* uo = (uint32_t*)o_; int32_t* io = (int32_t*)o_; \
    (void)a; (void)b; (void)c; (void)o; (void)ua; (void)ub; (void)ib; (void)uo; (void)io; (void)k;  \
    for (size_t i = 0; i < (size_t)n; ++i) { __VA_ARGS__ }                                          \
    return 0;                                                                                       \
  }

PROBE(p_fsqrtr, o[i] = rsqrt_(a[i]);)
PROBE(p_frintr, o[i] = rrint(a[i]);)
PROBE(p_ffloorr, o[i] = R(floor)(a[i]);)
PROBE(p_fclamp_pm, o[i] = rclamp(a[i], -b[i], b[i]);)
PROBE(p_fclampr_pm, o[i] = rclamp(a[i], -b[i], b[i]);)
PROBE(p_fdiv, o[i] = a[i] / b[i];)
PROBE(p_frcp, o[i] = R(1.0) / a[i];)
PROBE(p_fma, o[i] = rfma(a[i], b[i], c[i]);)
PROBE(p_sincosr, rsincos(a[i], o + 2 * i, o + 2 * i + 1);)
PROBE(p_atan_pos, o[i] = ratan_pos(a[i]);)
PROBE(p_atan2r, o[i] = ratan2(a[i], b[i]);)
PROBE(p_qmul, qmul(o + 4 * i, a + 4 * i, b + 4 * i);)
PROBE(p_qnormalize, for (int j = 0; j < 4; ++j) o[4 * i + j] = a[4 * i + j]; qnormalize(o + 4 * i);)
PROBE(p_qrotv, qrotv(o + 3 * i, a + 4 * i, b + 3 * i);)
PROBE(p_qmat, qmat(o + 9 * i, a + 4 * i);)
/* (the oracle has no qaxis_z of its own: it reads the third column of qmat) */
PROBE(p_qaxis_z, real m[9]; qmat(m, a + 4 * i); o[3 * i] = m[2]; o[3 * i + 1] = m[5]; o[3 * i + 2] = m[8];)
PROBE(p_mulv, m3mulv(o + 3 * i, a + 9 * i, b + 3 * i);)
PROBE(p_tmulv, m3tmulv(o + 3 * i, a + 9 * i, b + 3 * i);)
PROBE(p_mulv_mem, m3mulv(o + 3 * i, a + 9 * i, b + 3 * i);)
PROBE(p_tmulv_mem, m3tmulv(o + 3 * i, a + 9 * i, b + 3 * i);)
PROBE(p_euler_to_quat, euler_to_quat(o + 4 * i, a[3 * i], a[3 * i + 1], a[3 * i + 2]);)
PROBE(p_quat_to_euler, quat_to_euler(a + 4 * i, o + 3 * i);)
PROBE(p_quat_yaw, o[i] = quat_yaw(a + 4 * i);)
PROBE(p_philox, philox4x32_10(ua + 4 * i, ub + 2 * i, uo + 4 * i);)
#define PROBE_RNG orc_rng g; rng_init(&g, ua[5 * i], ua[5 * i + 1], ua[5 * i + 2], ua[5 * i + 3], ua[5 * i + 4]);
PROBE(p_rng_uniform01, PROBE_RNG for (int j = 0; j < k; ++j) o[i * k + j] = rng_uniform01(&g);)
PROBE(p_rng_uniform, PROBE_RNG for (int j = 0; j < k; ++j) o[i * k + j] = rng_uniform(&g, b[i], c[i]);)
PROBE(p_rng_randint, PROBE_RNG for (int j = 0; j < k; ++j) io[i * k + j] = rng_randint(&g, ib[i]);)
