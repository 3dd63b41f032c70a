// rv_dev_state.h -- whole env states as data: save, restore, branch (rv_state_save / rv_state_load / rv_branch) and
// the record of a simulated plan step (rv_plan_simulate).  Included by rv_kernels.hip only.
//
// A DevEnv block holds no pointer and no env id; every random draw of the env program is stateless Philox keyed by
// (seed, global env id, stream, reset_count | macro_index), and an env.step() with given actions draws nothing.  The
// pending partial step (in_step, step_stage, ms_*) lives in the block too.  Copying the block therefore IS copying
// the env: the kernels here move words and know nothing of what they mean.
//
// What a block does NOT hold and so is neither saved nor branched: the world's auto_reset switch, its stream, the
// statistics buffer and the task-queue buffers.  q_seq / q_sum (the hand-over stamp of the last queued rollout) travel
// with the block and are harmless: the first task an env gets in a queued launch is not checked against them
// (rv_env_kernel.h, rv_env_task: `k0 > 0`), and every later task sees what the launch itself stored.
#ifndef RV_DEV_STATE_H_
#define RV_DEV_STATE_H_
#include "rv_dev_env_types.h"

// (the kernels here are at file scope.  rv_kernels.hip, the only includer, says `using namespace rv` before it includes
// this header; the include above and this declaration are what lets the header compile on its own)
using rv::DevEnv;

#define RV_STATE_TPB 256
#define RV_STATE_WORDS ((int)(sizeof(DevEnv) / 4))
// a block is a whole number of 16-byte pieces: then block k of a 16-byte aligned base is 16-byte aligned as well
#define RV_STATE_VEC_OK (sizeof(DevEnv) % 16 == 0)
// 1: the identity, unmasked copies (rv_state_save, rv_state_load without an index) are the runtime's device-to-device
// copy; 0: the gather kernel.  Measured (profiles/state_branch_bench.txt): the runtime's copy is the
// faster of the two at every size tried, so identity goes through it
#define RV_STATE_IDENTITY_BY_RUNTIME 1

// Destination-major gather of env blocks: blockIdx.y (+ j0) is the destination block j, the RV_STATE_TPB threads of its one
// workgroup stride over its words -- every thread asks for all its pieces first and stores them afterwards, so a wave has
// its whole share of the block in flight at once.  The source block is index[j] (NULL: j / s -- s = 1 is the identity,
// s > 1 fans every source block out to s destinations, whose s readers of one source block hit the L2).  A source index
// outside [0, n_src) leaves block j untouched; nothing outside the two arrays is ever addressed.  V4: 16-byte accesses
// (both bases 16-byte aligned and RV_STATE_VEC_OK, checked by the launcher), dwords otherwise.  No LDS.
// (piece U of the thread, then the later pieces, then its store: written without an array, which the compiler would
// otherwise move into LDS)
template <typename T, int COUNT, int U>
struct StateBlockCopy {
  static __device__ __forceinline__ void run(T* __restrict__ b, const T* __restrict__ a) {
    const int i = (int)threadIdx.x + U * RV_STATE_TPB;
    if (i < COUNT) {
      const T v = a[i];
      StateBlockCopy<T, COUNT, U + 1>::run(b, a);
      b[i] = v;
    }
  }
};
template <typename T, int COUNT>
struct StateBlockCopy<T, COUNT, (COUNT + RV_STATE_TPB - 1) / RV_STATE_TPB> {
  static __device__ __forceinline__ void run(T* __restrict__, const T* __restrict__) {}
};
template <typename T, int COUNT>
__device__ __forceinline__ void state_block_copy(T* __restrict__ b, const T* __restrict__ a) { StateBlockCopy<T, COUNT, 0>::run(b, a); }
template <bool V4>
__global__ __launch_bounds__(RV_STATE_TPB) void k_env_blocks_gather(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src,
                                                                    int j0, int n_dst, int n_src, const int32_t* __restrict__ index, int s) {
  const int j = j0 + (int)blockIdx.y;
  if (j >= n_dst) return;
  const int k = index ? index[j] : j / s;
  if (k < 0 || k >= n_src) return;
  const size_t W = (size_t)RV_STATE_WORDS;
  if (V4) state_block_copy<uint4, RV_STATE_WORDS / 4>(reinterpret_cast<uint4*>(dst + (size_t)j * W), reinterpret_cast<const uint4*>(src + (size_t)k * W));
  else state_block_copy<uint32_t, RV_STATE_WORDS>(dst + (size_t)j * W, src + (size_t)k * W);
}

// rv_plan_simulate, before step t: env j of the plan world takes the actions of step t of its plan, actions [n][h][G][4]
// (n = N * s branch envs, env-major as the plan world is)
__global__ void k_plan_actions(DevEnv* envs, int n, const float* __restrict__ actions, int G, int h, int t) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * G * 4) return;
  const int j = i / (G * 4), r = i % (G * 4);
  envs[j].action[r / 4][r % 4] = actions[((size_t)j * h + t) * G * 4 + r];
}

// rv_plan_simulate, after step t: one thread per (branch env, body).  states [n][h][RV_MAXB][2] takes the xy of the
// env's observation (obs_pos: zeros for bodies that are not there, as PoseObs gives them), rewards / dones [n][h] what
// rv_reward reports: the reward of the step (0 where the launch skipped the env: its episode was over) and done.  An
// env that was skipped kept its observation, so its row repeats its last state.
__global__ void k_plan_record(const DevEnv* envs, int n, int h, int t, float* __restrict__ states, float* __restrict__ rewards, uint8_t* __restrict__ dones) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n * RV_MAXB) return;
  const int j = i / RV_MAXB, b = i % RV_MAXB;
  const DevEnv& e = envs[j];
  const size_t row = (size_t)j * h + t;
  if (states) {
    float2 xy; xy.x = e.obs_pos[b][0]; xy.y = e.obs_pos[b][1];
    reinterpret_cast<float2*>(states)[row * RV_MAXB + b] = xy;
  }
  if (b == 0) {
    if (rewards) rewards[row] = e.reward_valid ? e.last_reward : 0.0f;
    if (dones) dones[row] = (uint8_t)(e.done != 0);
  }
}

#endif  // RV_DEV_STATE_H_
