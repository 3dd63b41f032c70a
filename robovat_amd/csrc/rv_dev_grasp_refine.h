// rv_dev_grasp_refine.h -- the step between two scorings of a cross-entropy refinement of grasp candidates
// (rv_grasp_refine, include/rovat.h): rank an env's K candidates by their scores, keep the elites, and
// write the next generation around them, with the sampler's own validity checks and the world actions.  A stand-alone
// kernel beside the env program, like rv_dev_grasp_quality.h; it includes rv_dev_env.h for DevEnv (the calibration) and
// RV_DEV, rv_dev_grasp_sampler.h for step 8 and the 4-DoF conversion, rv_dev_cem.h for the normals and the ranking key.
//
// Everything below is float32, every product and every sum rounded on its own (-ffp-contract=off, as in rv_grasp_crops);
// the only fused operations are the two inside sincosr next to a zero.
//
// Candidates.  Input row j of env n, [x1, y1, x2, y2, z], is a candidate when (d_status is NULL or status[n] == RV_AP_OK)
// and (d_count is NULL or j < count[n]); with both NULL every row is one.  V = the number of candidates of the env.
//
// Ranking.  The total order of k_cem_refit (rv_dev_cem.h (a)) over the candidates: the word (cem_key(score) << 32) | j,
// ascending -- descending scores, the lower index first among equals, +0 and -0 equal, NaNs after every number and by
// index.  The rank of a candidate is the number of candidates whose word is smaller.  E' = min(n_elites, V).
//
// Output row j of env n:
//   V = 0:       input row j, bit for bit; parent[j] = j; count_out = 0.
//   j <  E':     the candidate of rank j, bit for bit; parent[j] = its input index.
//   j >= E':     a child of the candidate of rank r = (j - E') mod E', input index e, row [x1, y1, x2, y2, z]:
//     (z0, z1) = normal_pair(o0, o1), (z2, z3) = normal_pair(o2, o3) of the Philox block below (|z| <= 5.77)
//     gx = 0.5 * (x1 + x2);  gy = 0.5 * (y1 + y2)              the parent's centre
//     ax = 0.5 * (x2 - x1);  ay = 0.5 * (y2 - y1)              its half axis
//     cx = gx + sigma_center * z0;  cy = gy + sigma_center * z1
//     (s, c) = sincosr(sincos_arg(sigma_angle * z2))           (the clamp to |.| <= 1e4 only matters for a huge sigma)
//     bx = c * ax - s * ay;  by = s * ax + c * ay              the half axis rotated: no arctangent, the length changes
//                                                              only by rounding
//     child = [cx - bx, cy - by, cx + bx, cy + by, .]
//     ux = 0.5 * (child x1 + child x2);  uy likewise           the centre OF THE ROW AS WRITTEN -- the one rv_grasp_crops
//                                                              and ap_grasp_4dof will form from it; it is what is checked
//     inside = ux >= c0 && ux <= c0 + Wc && uy >= r0 && uy <= r0 + Hc      decided in float, false for NaN: the
//              sampler's centres lie between two crop pixels, a child's need not, and |.| in the distance below would
//              pass a centre far outside; it also keeps every integer formed after it small
//     step 8 of rv_dev_grasp_sampler.h on the UNFILTERED image at (ux, uy), by that header's ap_check_center: the
//              distance from the crop boundary >= MIN_DIST_FROM_BOUNDARY, and cd = the minimum over
//              [int(uy - WH), int(uy + WH)) x [int(ux - WW), int(ux + WW)) neither 0 nor NaN
//     lo = cd + MIN_DEPTH_OFFSET;  hi = cd + MAX_DEPTH_OFFSET
//     child z = fclampr(z + sigma_depth * z3, lo, hi)           (x < lo ? lo : x > hi ? hi : x; a NaN stays a NaN)
//     accepted = inside && step 8 && all five floats finite (|v| <= FLT_MAX)
//     accepted:  the child's row, parent[j] = e.   Otherwise: the parent's row, bit for bit, parent[j] = -1 - e.
//   count_out = K when V > 0.
// Re-checking antipodality or force closure is not done: the children leave the edge pixels by design.
// actions4 row j (when asked for) = ap_grasp_4dof of OUTPUT row j with the env's own calibration -- the conversion
// k_policy_antipodal_multi applies, so a row copied from that kernel's output gets that kernel's action bit for bit.
//
// Keys.  One Philox4x32-10 block per output row gives its four normals.  Key = the world's seed (seed_lo, seed_hi),
// counter words
//   c0 = (iteration << 6) | j             iteration in [0, 2^26), j < RV_AP_MAX_SAMPLES = 64 = 2^6
//   c1 = the policy's seed (rv_grasp_refine_params.seed)
//   c2 = global env id (env_id_offset + n)
//   c3 = (RV_STREAM_GRASP_REFINE << 24) | macro_index      macro_index in [0, 2^24)
// -- a function of nothing else: not of N, K, n_elites or the other envs.  The components 0 .. 3 are the block's four
// output words.  c3 cannot meet another stream's: the ids are distinct (the table of RV_STREAM_* in
// rv_dev_math.h).  Arguments outside the ranges are refused.
//
// Buffers and contract (rv_grasp_refine in rv_kernels.hip).  d_depth [N][H][W]; d_grasps [N][K][5] as
// rv_policy_antipodal_multi or an earlier call wrote them; d_scores [N][K]; d_count, d_status [N] or NULL; d_grasps_out
// [N][K][5], not d_grasps; d_actions4_out [N][K][4] or NULL (a grasp world only); d_parent [N][K] or NULL; d_count_out [N]
// or NULL.  h_sampler supplies use_crop, crop, min_dist_from_boundary, depth_sample_window_height / _width,
// min_depth_offset and max_depth_offset and nothing else.  Without actions4 any world will do: it supplies N, the global
// env ids, the seed, the device and the stream.  Asynchronous on the world's stream.  RV_ERR_VALUE before any launch, every
// output untouched: a NULL required pointer; a buffer that is not 4-byte aligned; d_grasps_out == d_grasps; K outside
// [1, RV_AP_MAX_SAMPLES]; n_elites outside [1, K]; height or width < 1; a sigma that is negative or not finite;
// macro_index or iteration outside the ranges above; a nonzero reserved word; sampler parameters that
// rv_policy_antipodal_multi would refuse (one host function checks them for both); d_actions4_out on a push world.
//
// Shape: one wave64 per env, lane j holds row j (K <= 64), four envs per workgroup of 256; no LDS, no atomics, no
// barrier.  The rank is a count over K wave-uniform readlanes of (key, candidate) pairs; the elite of rank r is found by
// a ballot, and a lane fetches its parent's five floats with five bpermutes.  The depth-window minimum is a per-lane gather
// over at most 2 WH x 2 WW pixels served by the caches.  The outputs leave by ordinary per-lane vector stores, row by
// row (20 and 16 bytes a lane, neighbouring lanes neighbouring rows).  Every global index is a size_t.  No env state is
// read beyond the calibration (and that only for actions4), none is written.
// tests/grasp_refine_host.py restates this header in float32 NumPy, operation for operation; the GPU tests compare the
// rows, parents and counts bit for bit (the yaw of actions4 goes through libm's atan2f / cosf / sinf on the device and is
// compared within a bound).
#ifndef RV_DEV_GRASP_REFINE_H_
#define RV_DEV_GRASP_REFINE_H_
#include "rv_dev_env.h"
#include "rv_dev_grasp_sampler.h"
#include "rv_dev_cem.h"

#define RV_GR_MAX_ITERATION (1 << 26)
#define RV_GR_MAX_MACRO_INDEX (1 << 24)
#define RV_GR_TPB 256

namespace rv {
struct GrArgs {
  rv_grasp_refine_params p;
  ApArgs ap;                // the sampler's checks: p, depth, H, W, r0, c0, Hc, Wc (nothing else of it is read)
  const float* grasps;      // [N][K][5]
  const float* scores;      // [N][K]
  const int32_t* count;     // [N] or null
  const int32_t* status;    // [N] or null
  float* grasps_out;        // [N][K][5]
  float* actions4;          // [N][K][4] or null
  int32_t* parent;          // [N][K] or null
  int32_t* count_out;       // [N] or null
  int K;
};
RV_DEV bool gr_finite(float v) { return fabsr(v) <= 3.402823466e38f; }
// the child of parent row g for the normals z; false: not accepted (out is then not to be used)
RV_DEV bool gr_child(const GrArgs& a, const float* img, const float (&g)[5], const float (&z)[4], float (&out)[5]) {
  const rv_grasp_refine_params& p = a.p;
  const float gx = 0.5f * (g[0] + g[2]), gy = 0.5f * (g[1] + g[3]);
  const float ax = 0.5f * (g[2] - g[0]), ay = 0.5f * (g[3] - g[1]);
  const float cx = gx + p.sigma_center * z[0], cy = gy + p.sigma_center * z[1];
  float s, c;
  sincosr(sincos_arg(p.sigma_angle * z[2]), &s, &c);
  const float bx = c * ax - s * ay, by = s * ax + c * ay;
  out[0] = cx - bx; out[1] = cy - by; out[2] = cx + bx; out[3] = cy + by;
  const float ux = 0.5f * (out[0] + out[2]), uy = 0.5f * (out[1] + out[3]);
  const ApArgs& A = a.ap;
  const bool inside = ux >= (float)A.c0 && ux <= (float)(A.c0 + A.Wc) && uy >= (float)A.r0 && uy <= (float)(A.r0 + A.Hc);
  if (!inside) return false;
  float cd;
  if (!ap_check_center(A, img, ux, uy, &cd)) return false;
  const float lo = cd + A.p.min_depth_offset, hi = cd + A.p.max_depth_offset;
  out[4] = fclampr(g[4] + p.sigma_depth * z[3], lo, hi);
  return gr_finite(out[0]) && gr_finite(out[1]) && gr_finite(out[2]) && gr_finite(out[3]) && gr_finite(out[4]);
}
}  // namespace rv

#if RV_ON_DEVICE
__global__ __launch_bounds__(RV_GR_TPB) void k_grasp_refine(const rv::DevEnv* envs, int n, const rv_config* c, rv::GrArgs a) {
  using namespace rv;
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (RV_GR_TPB / 64) + (threadIdx.x >> 6)));
  if (i >= n) return;
  const int K = a.K;
  const bool row = lane < K;
  const size_t at = (size_t)i * (size_t)K + (size_t)lane;
  float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t key = 0xffffffffu;
  bool cand = row && (!a.status || a.status[i] == RV_AP_OK) && (!a.count || lane < a.count[i]);
  if (row) {
#pragma unroll
    for (int k = 0; k < 5; ++k) g[k] = a.grasps[at * 5 + (size_t)k];
    if (cand) key = cem_key(a.scores[at]);
  }
  const unsigned long long cmask = __ballot(cand);
  const int V = __popcll(cmask);
  if (lane == 0 && a.count_out) a.count_out[i] = V > 0 ? K : 0;
  // (the lanes past K take part in the wave-wide operations below and store nothing)
  float out[5] = {g[0], g[1], g[2], g[3], g[4]};
  int par = lane;
  if (V > 0) {
    // rank: the candidates whose (key, index) word is smaller than mine
    int rank = 0;
    for (int l = 0; l < K; ++l) {
      const uint32_t kl = (uint32_t)__builtin_amdgcn_readlane((int)key, l);
      const bool cl = ((cmask >> l) & 1ull) != 0ull;
      rank += (cl && (kl < key || (kl == key && l < lane))) ? 1 : 0;
    }
    const int Ep = a.p.n_elites < V ? a.p.n_elites : V;
    const int r = lane < Ep ? lane : (lane - Ep) % Ep;
    // the input index of the elite of rank r
    int e = 0;
    for (int q = 0; q < Ep; ++q) {
      const unsigned long long m = __ballot(cand && rank == q);      // (exactly one lane: the order is total)
      const int el = __ffsll((long long)m) - 1;
      if (r == q) e = el;
    }
    float pg[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) pg[k] = __shfl(g[k], e, 64);
#pragma unroll
    for (int k = 0; k < 5; ++k) out[k] = pg[k];
    par = e;
    if (row && lane >= Ep) {
      uint32_t o0, o1, o2, o3;
      philox(((uint32_t)a.p.iteration << 6) | (uint32_t)lane, a.p.seed, (uint32_t)(c->env_id_offset + i),
             (RV_STREAM_GRASP_REFINE << 24) | (uint32_t)a.p.macro_index, c->seed_lo, c->seed_hi, &o0, &o1, &o2, &o3);
      float z[4], ch[5];
      normal_pair(o0, o1, &z[0], &z[1]);
      normal_pair(o2, o3, &z[2], &z[3]);
      const float* img = a.ap.depth + (size_t)i * (size_t)a.ap.H * (size_t)a.ap.W;
      if (gr_child(a, img, pg, z, ch)) {
#pragma unroll
        for (int k = 0; k < 5; ++k) out[k] = ch[k];
      } else {
        par = -1 - e;
      }
    }
  }
  if (!row) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) a.grasps_out[at * 5 + (size_t)k] = out[k];
  if (a.parent) a.parent[at] = par;
  if (a.actions4) {
    const DevEnv& env = envs[i];
    float a4[4];
    ap_grasp_4dof(env.cam_intrinsics, env.cam_rotation, env.cam_translation, out, a4);
#pragma unroll
    for (int k = 0; k < 4; ++k) a.actions4[at * 4 + (size_t)k] = a4[k];
  }
}
#endif  // RV_ON_DEVICE
#endif
