// rv_dev_cem.h — the two kernels of a cross-entropy-method planner (rv_cem_sample / rv_cem_refit).
//
// A planner keeps, per env, a normal distribution over plans of H steps: mean[D] and std[D], D = H * A floats,
// A = 4 * max(NUM_GOAL_STEPS, 1).  rv_cem_sample draws S candidates from it, rv_cem_refit fits it to the E candidates
// with the largest returns.  Everything below is float32, every product and every sum rounded on its own
// (-ffp-contract=off), except where rv_fma is written.
//
// logr(x), x in (0, 1] and normal (every caller passes k * 2^-24, k = 1 .. 2^24):
//   the classic split x = 2^k * m with m in [sqrt(1/2), sqrt(2)) by integer arithmetic on the bits (bits + 0x3f800000 -
//   0x3f3504f3; k = (that >> 23) - 127; the low 23 bits + 0x3f3504f3 are m), f = m - 1 (exact), s = f / (2 + f),
//   z = s * s, w = z * z, R = z * (L1 + w * L3) + w * (L2 + w * L4) (the atanh series 2 s + 2/3 s^3 + ... folded into a
//   minimax polynomial, the coefficients of FreeBSD's e_logf.c), hfsq = (0.5 * f) * f, and
//   log x = ((((s * (hfsq + R) + k * LN2_LO) - hfsq) + f) + k * LN2_HI, LN2_HI + LN2_LO = ln 2 with k * LN2_HI exact.
//   CONTRACT (measured over all 2^24 inputs k * 2^-24 against float64, tests/test_cem_host.py): the error is
//   <= 1 ulp of the true value (measured 0.83, at x = 0.702913), and <= 2^-24 absolute for x >= 1/2, where |log x| < 0.7
//   (measured 3.94e-8); logr(1) = 0 exactly.
//
// normal_pair(a, b) from two Philox words (Box-Muller):
//   u1 = (float)((a >> 8) + 1) * 2^-24            in (0, 1]
//   u2 = (float)(b >> 8) * 2^-24                  in [0, 1)    (rng_uniform01)
//   r  = fsqrtr(-2 * logr(u1))                    r <= fsqrtr(48 ln 2) = 5.7681 <= 5.77: no normal lies beyond that
//   (sn, cs) = sincosr(RV_CEM_TWO_PI * u2)        the angle is in [0, 6.2832] -- inside |x| <= 26, where sincosr is
//                                                 within 2 ulp of the true value
//   z0 = r * cs, z1 = r * sn
//
// Keys.  One Philox4x32-10 block (o0 .. o3) gives the four normals of candidate j, d = 4 q .. 4 q + 3:
// (z[4q], z[4q+1]) = normal_pair(o0, o1), (z[4q+2], z[4q+3]) = normal_pair(o2, o3).  Key = the world's seed (seed_lo,
// seed_hi), counter words
//   c0 = (iteration << 17) | (j << 7) | q        iteration in [0, 2^15), j < 1024 = 2^10, q = d / 4 < 128 = 2^7
//   c1 = the policy's seed (rv_cem_params.seed)
//   c2 = global env id (env_id_offset + n)
//   c3 = (RV_STREAM_CEM << 24) | plan_index      plan_index in [0, 2^24)
// -- a function of nothing else: not of N, S, H or of the other envs of the world.  c3 cannot meet another stream's: the ids
// are distinct (the table of RV_STREAM_* in rv_dev_math.h).  Arguments outside the ranges are refused.
//
// k_cem_sample: one lane per (n, j, q); x[n][j][d] = fclampr(mean[n][d] + std[n][d] * z[d], -1, 1) (the product rounded,
// then the sum); with keep_mean, candidate 0 is fclampr(mean[n][d], -1, 1) and draws nothing.  x is [N][S][H][G][4], the
// d_actions of rv_plan_simulate; a lane stores its four floats as one float4 (16-byte aligned buffers) or as four floats,
// neighbouring lanes neighbouring q.
//
// k_cem_refit: one workgroup per env, 64 / 256 / 1024 threads for S <= 64 / <= 256 / more (k_plan_score's shapes).
//  (a) rank.  A return r becomes the uint32 key  NaN -> 0xffffffff;  otherwise b = bits(r), -0 taken as +0,
//      key = ~(b ^ (b >> 31 ? 0xffffffff : 0x80000000)): larger return, smaller key; -inf has key 0xff800000, below NaN's.
//      The word (key << 32) | j is unique per candidate; the S words, padded with ~0 to a power of two >= 64, are sorted
//      ascending in LDS by a bitonic network.  Hence: descending returns, the lower index first among equals, +-0 equal,
//      NaNs last and by index -- a total order that does not depend on the schedule.
//  (b) the elites e_0 .. e_{E-1} are the low words of the first E entries; they stay in LDS and go to d_elite[N][E] when
//      that is given.
//  (c) thread t takes d = t, t + T, ...:
//      sum = 0; for k in 0 .. E-1 (rank order): sum = sum + x[n][e_k][d];        m = sum / (float)E
//      v = 0;   for k in 0 .. E-1: dl = x[n][e_k][d] - m; v = v + dl * dl;        v = v / (float)E;  sd = fsqrtr(v)
//      mean'[d] = alpha * mean[d] + oma * m;  std'[d] = fmaxr(alpha * std[d] + oma * sd, min_std);  oma = 1 - alpha, once
//      Neighbouring threads read neighbouring d of the same candidate (the second pass finds the rows in the caches).
//      mean / std are updated in place, each [d] by the thread that read it.
// tests/cem_host.py restates this header in float32 NumPy, operation for operation; the GPU tests compare bit for bit.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"

namespace rv {

#define RV_CEM_MAX_TPB 1024
#define RV_CEM_MAX_ITERATION (1 << 15)
#define RV_CEM_MAX_PLAN_INDEX (1 << 24)
#define RV_CEM_TWO_PI 6.283185307179586f

RV_DEV float logr(float x) {
  uint32_t ix = __builtin_bit_cast(uint32_t, x);
  ix += 0x3f800000u - 0x3f3504f3u;
  const int k = (int)(ix >> 23) - 127;
  ix = (ix & 0x007fffffu) + 0x3f3504f3u;
  const float f = __builtin_bit_cast(float, ix) - 1.0f;
  const float s = f / (2.0f + f);
  const float z = s * s, w = z * z;
  const float t1 = w * (0.40000972152f + w * 0.24279078841f);
  const float t2 = z * (0.66666662693f + w * 0.28498786688f);
  const float R = t2 + t1;
  const float hfsq = (0.5f * f) * f;
  const float dk = (float)k;
  return (((s * (hfsq + R) + dk * 9.0580006145e-6f) - hfsq) + f) + dk * 6.9313812256e-1f;
}

RV_DEV void normal_pair(uint32_t a, uint32_t b, float* z0, float* z1) {
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
  const float r = fsqrtr(-2.0f * logr(u1));
  float sn, cs;
  sincosr(RV_CEM_TWO_PI * u2, &sn, &cs);
  *z0 = r * cs; *z1 = r * sn;
}

// the four normals of (env gid, candidate j, floats 4 q .. 4 q + 3)
RV_DEV void cem_normals(uint32_t seed_lo, uint32_t seed_hi, uint32_t gid, const rv_cem_params& p, int j, int q, float (&z)[4]) {
  uint32_t o0, o1, o2, o3;
  philox(((uint32_t)p.iteration << 17) | ((uint32_t)j << 7) | (uint32_t)q, p.seed, gid,
         (RV_STREAM_CEM << 24) | (uint32_t)p.plan_index, seed_lo, seed_hi, &o0, &o1, &o2, &o3);
  normal_pair(o0, o1, &z[0], &z[1]);
  normal_pair(o2, o3, &z[2], &z[3]);
}

// the sort key of a return: see (a) above
RV_DEV uint32_t cem_key(float r) {
  if (r != r) return 0xffffffffu;
  uint32_t b = __builtin_bit_cast(uint32_t, r);
  if (b == 0x80000000u) b = 0u;
  return ~(b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u));
}

#if RV_ON_DEVICE
struct CemArgs {
  rv_cem_params p;
  const float* actions;     // refit: [N][S][D]
  const float* returns;     // refit: [N][S]
  float* mean; float* std;  // [N][D] (sample: read only)
  float* out;               // sample: [N][S][D]
  int32_t* elite;           // refit: [N][E] or null
  int S, D;
};

template <bool V4>
__global__ __launch_bounds__(256) void k_cem_sample(const rv_config* cfg, CemArgs a, long long total) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int D4 = a.D >> 2;
  const int q = (int)(t % D4);
  const long long row = t / D4;      // n * S + j
  const int j = (int)(row % a.S), n = (int)(row / a.S);
  const float* mean = a.mean + (size_t)n * a.D + 4 * q;
  const float* std = a.std + (size_t)n * a.D + 4 * q;
  float x[4];
  if (a.p.keep_mean && j == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = fclampr(mean[k], -1.0f, 1.0f);
  } else {
    float z[4];
    cem_normals(cfg->seed_lo, cfg->seed_hi, (uint32_t)(cfg->env_id_offset + n), a.p, j, q, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = fclampr(mean[k] + std[k] * z[k], -1.0f, 1.0f);
  }
  float* o = a.out + (size_t)row * a.D + 4 * q;
  if constexpr (V4) {
    *reinterpret_cast<float4*>(o) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = x[k];
  }
}

__global__ __launch_bounds__(RV_CEM_MAX_TPB) void k_cem_refit(CemArgs a) {
  __shared__ unsigned long long s_word[RV_CEM_MAX_SAMPLES];
  const int tid = (int)threadIdx.x, T = (int)blockDim.x, n = (int)blockIdx.x;
  const int S = a.S, D = a.D, E = a.p.n_elites;
  int m = 64; while (m < S) m <<= 1;
  for (int t = tid; t < m; t += T)
    s_word[t] = t < S ? (((unsigned long long)cem_key(a.returns[(size_t)n * S + t]) << 32) | (unsigned long long)t) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < m; t += T) {
        const int u = t ^ j;
        if (u > t) {
          const unsigned long long x = s_word[t], y = s_word[u];
          if ((x > y) == ((t & k) == 0)) { s_word[t] = y; s_word[u] = x; }
        }
      }
      __syncthreads();
    }
  if (a.elite)
    for (int k = tid; k < E; k += T) a.elite[(size_t)n * E + k] = (int32_t)(uint32_t)s_word[k];
  const float* x = a.actions + (size_t)n * S * D;
  const float fe = (float)E, alpha = a.p.alpha, oma = 1.0f - alpha;
  for (int d = tid; d < D; d += T) {
    float sum = 0.0f;
#pragma unroll 4
    for (int k = 0; k < E; ++k) sum += x[(size_t)(uint32_t)s_word[k] * D + d];
    const float mu = sum / fe;
    float v = 0.0f;
#pragma unroll 4
    for (int k = 0; k < E; ++k) { const float dl = x[(size_t)(uint32_t)s_word[k] * D + d] - mu; v += dl * dl; }
    v = v / fe;
    const float sd = fsqrtr(v);
    const size_t at = (size_t)n * D + d;
    const float m0 = a.mean[at], s0 = a.std[at];
    a.mean[at] = alpha * m0 + oma * mu;
    a.std[at] = fmaxr(alpha * s0 + oma * sd, a.p.min_std);
  }
}
#endif  // RV_ON_DEVICE

}  // namespace rv
