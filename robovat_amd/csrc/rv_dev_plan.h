// rv_dev_plan.h — planning-mode PushReward on the device (rv_plan_reward / rv_plan_score).
//
// Reference chain (StanfordVL/robovat), get_reward_fn(task, layout, is_planning=True)(state, next_state):
//   check_stride                       robovat/reward_fns/push_reward.py:230-238, 312-323
//   check_border / check_target_border push_reward.py:241-269, 325-331
//   insertion_termination              push_reward.py:110-151
//   crossing_termination               push_reward.py:168-200
//   goal / penalty / dense / time      push_reward.py:338-370
//
// One transition (state -> next_state, B bodies, xy each), in float32 and in this order:
//  1. stride  |next_b - state_b| per body; terminated when ALL are below the minimum or ANY is above the maximum
//             (0.01 / 0.15, high level 0.1 / 0.3)
//  2. border  any body of next_state outside [0.22 - 0.02, 0.98 + 0.02] x [-0.56 - 0.02, 0.66 + 0.02]; insertion: body 0
//             also outside x in [0.3 - 0.02, 0.8 + 0.02]
//  3. middle  m1 = state + (1/3) (next - state), m2 = state + (2/3) (next - state)
//     insertion: terminated when any body's next, m1 or m2 lies on a region tile of size 1.25 x size (the tile CENTRES
//                move with the size too: offset + tile * 1.25 size)
//     crossing:  terminated unless body 0's next, m1 and m2 all lie on region tiles (max_dist = size)
//     clearing:  no termination function
//  4. goal    clearing: no body of next_state on a 1.25 x region tile; otherwise body 0 of next_state on a goal tile;
//             masked by the termination.  The penalty is the termination itself (planning mode does not mask it by the goal)
//  5. reward  ((goal_reward * goal + termination_reward * penalty) + dense_reward * |score(next) - score(state)|) + time_reward
//             score: clearing -min(mean_b |x - 0.7|, mean_b |y + 0.9|) over the B bodies (the overwritten minimum of the
//             reference), otherwise -(distance of body 0 to the nearest goal tile centre)
//  6. termination = terminated or goal
// RV_TASK_NONE: reward 1, termination 0 (dummy_reward_fn).
//
// rv_plan_score walks the H steps of a plan in registers: ret += disc * r; stop after the first terminating step;
// disc *= gamma.  Launch shape: one workgroup per env, lanes over the S plans of that env (a lane takes plans lane,
// lane + blockDim, ...), so the arg-max of an env never leaves its workgroup: a wave shuffle reduction, then one pass
// over the per-wave winners in LDS.  The tile centres (both sizes) are computed once per workgroup into LDS; every
// lane reads them at wave-uniform addresses (broadcasts).  A lane loads its step record [B][2] as two float4 (B = 4,
// 16-byte aligned base) or as float2, and the record of step t + 1 is requested before step t is evaluated.
// tests/plan_host.py restates this header in float32 NumPy, operation for operation; the GPU tests compare bit for bit.
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_math.h"
#include "rv_dev_env.h"

namespace rv {

#define RV_PLAN_MAX_TPB 1024
#define RV_PLAN_MAX_WAVES (RV_PLAN_MAX_TPB / 64)

struct PlanArgs {
  rv_plan_params p;
  const float* state0;      // [N][B][2], or null: DevEnv::obs_pos
  const float* plans;       // [N][S][H][B][2]
  int S, H;
  float* returns;           // [N][S] or null
  int32_t* lengths;         // [N][S] or null
  int32_t* best;            // [N] or null
};

// the tile centres of the launch: region tiles at both sizes, goal tiles
struct PlanTiles {
  float region[RV_MAXTILES][2];       // offset + tile * size
  float region125[RV_MAXTILES][2];    // offset + tile * (1.25 size)
  float goal[RV_MAXTILES][2];
  float half, half125;                // 0.5 * max_dist of the two sizes
  int task, n_region, n_goal;
};

RV_DEV void plan_tiles_fill(PlanTiles& T, const rv_config* c, int tid) {
  const float size = c->tile_size, size125 = size * 1.25f;
  if (tid < RV_MAXTILES) {
    if (tid < c->n_region) {
      T.region[tid][0] = c->tile_offset[0] + c->region[tid][0] * size;
      T.region[tid][1] = c->tile_offset[1] + c->region[tid][1] * size;
      T.region125[tid][0] = c->tile_offset[0] + c->region[tid][0] * size125;
      T.region125[tid][1] = c->tile_offset[1] + c->region[tid][1] * size125;
    }
    if (tid < c->n_goal) {
      T.goal[tid][0] = c->tile_offset[0] + c->goal[tid][0] * size;
      T.goal[tid][1] = c->tile_offset[1] + c->goal[tid][1] * size;
    }
  }
  if (tid == 0) {
    T.half = 0.5f * size; T.half125 = 0.5f * size125;
    T.task = c->task;
    T.n_region = c->n_region < RV_MAXTILES ? c->n_region : RV_MAXTILES;
    T.n_goal = c->n_goal < RV_MAXTILES ? c->n_goal : RV_MAXTILES;
  }
}

RV_DEV int plan_on_tiles(float x, float y, const float (*centres)[2], int n, float half) {
  int on = 0;
  for (int i = 0; i < n; ++i)
    on |= (fabsr(x - centres[i][0]) <= half && fabsr(y - centres[i][1]) <= half) ? 1 : 0;
  return on;
}
RV_DEV float plan_goal_dist(float x, float y, const PlanTiles& T) {
  float best = 1e30f;
  for (int i = 0; i < T.n_goal; ++i) {
    const float dx = x - T.goal[i][0], dy = y - T.goal[i][1];
    const float d = fsqrtr(dx * dx + dy * dy);
    if (d < best) best = d;
  }
  return best;
}
template <int B>
RV_DEV float plan_score(const PlanTiles& T, const float (&s)[B][2]) {
  if (T.task == RV_TASK_CLEARING) {
    float d1 = 0.0f, d3 = 0.0f;
#pragma unroll
    for (int b = 0; b < B; ++b) { d1 += fabsr(s[b][0] - 0.7f); d3 += fabsr(s[b][1] + 0.9f); }
    d1 /= (float)B; d3 /= (float)B;
    return -fminr(d1, d3);
  }
  return -plan_goal_dist(s[0][0], s[0][1], T);
}

// the table border of check_border / check_target_border with its tolerance, rounded once from the float64 constants
#define RV_PLAN_X_LO  ((float)(0.22 - 0.02))
#define RV_PLAN_X_HI  ((float)(0.98 + 0.02))
#define RV_PLAN_Y_LO  ((float)(-0.56 - 0.02))
#define RV_PLAN_Y_HI  ((float)(0.66 + 0.02))
#define RV_PLAN_TX_LO ((float)(0.3 - 0.02))
#define RV_PLAN_TX_HI ((float)(0.8 + 0.02))
#define RV_PLAN_THIRD      ((float)(1.0 / 3.0))
#define RV_PLAN_TWO_THIRDS ((float)(2.0 / 3.0))

template <int B>
RV_DEV void plan_reward(const PlanTiles& T, const rv_plan_params& p, const float (&s)[B][2], const float (&n)[B][2],
                        float* reward, int* termination) {
  if (T.task == RV_TASK_NONE) { *reward = 1.0f; *termination = 0; return; }
  const float min_stride = p.is_high_level ? 0.1f : 0.01f, max_stride = p.is_high_level ? 0.3f : 0.15f;
  int all_small = 1, any_big = 0, outside = 0;
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const float dx = n[b][0] - s[b][0], dy = n[b][1] - s[b][1];
    const float stride = fsqrtr(dx * dx + dy * dy);
    all_small &= stride < min_stride ? 1 : 0;
    any_big |= stride > max_stride ? 1 : 0;
    outside |= (n[b][0] < RV_PLAN_X_LO || n[b][0] > RV_PLAN_X_HI || n[b][1] < RV_PLAN_Y_LO || n[b][1] > RV_PLAN_Y_HI) ? 1 : 0;
  }
  int term = all_small | any_big | outside;
  if (T.task == RV_TASK_INSERTION) {
    term |= (n[0][0] < RV_PLAN_TX_LO || n[0][0] > RV_PLAN_TX_HI || n[0][1] < RV_PLAN_Y_LO || n[0][1] > RV_PLAN_Y_HI) ? 1 : 0;
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float dx = n[b][0] - s[b][0], dy = n[b][1] - s[b][1];
      term |= plan_on_tiles(n[b][0], n[b][1], T.region125, T.n_region, T.half125);
      term |= plan_on_tiles(s[b][0] + RV_PLAN_THIRD * dx, s[b][1] + RV_PLAN_THIRD * dy, T.region125, T.n_region, T.half125);
      term |= plan_on_tiles(s[b][0] + RV_PLAN_TWO_THIRDS * dx, s[b][1] + RV_PLAN_TWO_THIRDS * dy, T.region125, T.n_region, T.half125);
    }
  } else if (T.task == RV_TASK_CROSSING) {
    const float dx = n[0][0] - s[0][0], dy = n[0][1] - s[0][1];
    int bridge = plan_on_tiles(n[0][0], n[0][1], T.region, T.n_region, T.half);
    bridge &= plan_on_tiles(s[0][0] + RV_PLAN_THIRD * dx, s[0][1] + RV_PLAN_THIRD * dy, T.region, T.n_region, T.half);
    bridge &= plan_on_tiles(s[0][0] + RV_PLAN_TWO_THIRDS * dx, s[0][1] + RV_PLAN_TWO_THIRDS * dy, T.region, T.n_region, T.half);
    term |= bridge ^ 1;
  }
  int goal;
  if (T.task == RV_TASK_CLEARING) {
    goal = 1;
#pragma unroll
    for (int b = 0; b < B; ++b) goal &= plan_on_tiles(n[b][0], n[b][1], T.region125, T.n_region, T.half125) ^ 1;
  } else {
    goal = plan_on_tiles(n[0][0], n[0][1], T.goal, T.n_goal, T.half);
  }
  goal &= term ^ 1;
  float r = 0.0f;
  r += p.goal_reward * (float)goal;
  r += p.termination_reward * (float)term;
  if (p.use_dense_reward) r += fabsr(plan_score<B>(T, n) - plan_score<B>(T, s)) * p.dense_reward;
  if (p.use_time_penalty) r += p.time_reward;
  *reward = r; *termination = term | goal;
}

// one record [B][2]: two float4 when B == 4 and the base is 16-byte aligned (V4), float2 otherwise
template <int B, bool V4>
RV_DEV void plan_load(const float* p, float (&o)[B][2]) {
  if constexpr (B == 4 && V4) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    o[0][0] = a.x; o[0][1] = a.y; o[1][0] = a.z; o[1][1] = a.w;
    o[2][0] = b.x; o[2][1] = b.y; o[3][0] = b.z; o[3][1] = b.w;
  } else {
#pragma unroll
    for (int b = 0; b < B; ++b) { const float2 v = reinterpret_cast<const float2*>(p)[b]; o[b][0] = v.x; o[b][1] = v.y; }
  }
}

// rv_plan_reward: one lane per transition
template <int B, bool V4>
__global__ __launch_bounds__(256) void k_plan_reward(const rv_config* cfg, rv_plan_params p, const float* state, const float* next_state,
                                                     long long m, float* reward, uint8_t* termination) {
  __shared__ PlanTiles T;
  plan_tiles_fill(T, cfg, (int)threadIdx.x);
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  float s[B][2], n[B][2];
  plan_load<B, V4>(state + i * (2 * B), s);
  plan_load<B, V4>(next_state + i * (2 * B), n);
  float r; int t;
  plan_reward<B>(T, p, s, n, &r, &t);
  reward[i] = r; termination[i] = (uint8_t)t;
}

// rv_plan_score: one workgroup per env (blockIdx.x), lanes over its S plans
template <int B, bool V4>
__global__ __launch_bounds__(RV_PLAN_MAX_TPB) void k_plan_score(const DevEnv* envs, const rv_config* cfg, PlanArgs a) {
  __shared__ PlanTiles T;
  __shared__ float s_val[RV_PLAN_MAX_WAVES];
  __shared__ int s_idx[RV_PLAN_MAX_WAVES];
  const int tid = (int)threadIdx.x, env = (int)blockIdx.x;
  plan_tiles_fill(T, cfg, tid);
  __syncthreads();
  float s0[B][2];
  if (a.state0) plan_load<B, false>(a.state0 + (size_t)env * (2 * B), s0);
  else {
#pragma unroll
    for (int b = 0; b < B; ++b) { s0[b][0] = envs[env].obs_pos[b][0]; s0[b][1] = envs[env].obs_pos[b][1]; }
  }
  // the best plan of this lane: the largest return, the lowest index among equals (a lane meets its plans in rising order)
  float best_v = 0.0f; int best_i = -1;
  for (int sidx = tid; sidx < a.S; sidx += (int)blockDim.x) {
    const size_t row = (size_t)env * (size_t)a.S + (size_t)sidx;
    const float* rec = a.plans + row * (size_t)a.H * (2 * B);
    float s[B][2], n[B][2], nn[B][2];
#pragma unroll
    for (int b = 0; b < B; ++b) { s[b][0] = s0[b][0]; s[b][1] = s0[b][1]; }
    plan_load<B, V4>(rec, n);
    float ret = 0.0f, disc = 1.0f; int len = a.H;
    for (int t = 0; t < a.H; ++t) {
      if (t + 1 < a.H) plan_load<B, V4>(rec + (size_t)(t + 1) * (2 * B), nn);      // (in flight while step t is evaluated)
      float r; int term;
      plan_reward<B>(T, a.p, s, n, &r, &term);
      ret += disc * r;
      if (term) { len = t + 1; break; }
      disc *= a.p.gamma;
      if (t + 1 < a.H) {
#pragma unroll
        for (int b = 0; b < B; ++b) { s[b][0] = n[b][0]; s[b][1] = n[b][1]; n[b][0] = nn[b][0]; n[b][1] = nn[b][1]; }
      }
    }
    if (a.returns) a.returns[row] = ret;
    if (a.lengths) a.lengths[row] = len;
    if (best_i < 0 || ret > best_v) { best_v = ret; best_i = sidx; }
  }
  if (!a.best) return;      // (uniform over the launch)
  // arg-max over the wave by shuffles (a lane without a plan has index -1 and never wins), then over the waves through LDS
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(best_v, o); const int i = __shfl_xor(best_i, o);
    if (i >= 0 && (best_i < 0 || v > best_v || (v == best_v && i < best_i))) { best_v = v; best_i = i; }
  }
  const int wave = tid >> 6, n_waves = ((int)blockDim.x + 63) >> 6;
  if ((tid & 63) == 0) { s_val[wave] = best_v; s_idx[wave] = best_i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < n_waves; ++w) {
      const float v = s_val[w]; const int i = s_idx[w];
      if (i >= 0 && (best_i < 0 || v > best_v || (v == best_v && i < best_i))) { best_v = v; best_i = i; }
    }
    a.best[env] = best_i;
  }
}

}  // namespace rv
