// rv_kernels.hip — __global__ kernels and the C ABI of librovat_hip.so
// (include/rovat.h).  gfx950 only; built with hipcc --offload-arch=gfx950.
//
// Kernel inventory:
//   k_env<MODE>     one wave64 per env, the whole reset / macro step / n
//                   substeps / settle loop out of LDS (rv_dev_env.h)
//   k_contact_points one wave64 per env: the PyBullet contact records (rv_dev_contacts.h)
//   k_plan_score    one workgroup per env, lanes over candidate plans: planning-mode PushReward (rv_dev_plan.h)
//   k_cem_sample    one lane per four floats of a candidate plan: keyed normal draws (rv_dev_cem.h)
//   k_cem_refit     one workgroup per env: rank the returns, refit mean / std to the elites (rv_dev_cem.h)
//   k_depth_noise_draw / k_depth_noise_apply   the depth sensor noise model: keyed per-image scalars and noise grid, then
//                   gamma multiplier + bicubic upsampling staged in LDS, one lane per pixel (rv_dev_depth_noise.h)
//   k_grasp_crops   grasp-centred depth crops per image grasp: a wave per 64 or 256 consecutive output pixels of one
//                   image, the grasp row wave-uniform, a nearest-neighbour gather (rv_dev_grasp_sampler.h)
//   k_grasp_quality the grasp-quality network: a workgroup per 8 crops, activations in LDS, conv2 / fc1 / fc2 on the
//                   f32 MFMA, conv1 / pose / logit as FMA chains on the VALU (rv_dev_grasp_quality.h)
//   k_gq_train_forward / k_gq_train_backward_sample / k_gq_train_backward_weights / k_adam_step   a training step of that
//                   network: the forward pass keeping its activations, a workgroup per sample for the data gradients and
//                   the convolutions' partial sums, a thread per weight for the chains over the batch, Adam per element
//                   (rv_dev_grasp_train.h)
//   k_deproject / k_segment_cloud   point clouds segmented without the segmask: a keyed plane fit, DBSCAN on LDS-resident
//                   points, the largest clusters sampled; one workgroup per env (rv_dev_segment.h)
//   k_ward_groups   exactly C groups of the clustered points: Ward agglomeration on the k-nearest-neighbour graph in float64,
//                   cluster moments and cached partners in LDS, adjacency as a bit matrix in the caller's workspace; one
//                   workgroup per env (rv_dev_ward.h)
//   k_*             small one-thread-per-env accessors behind the getters,
//                   setters, observation, reward and policy entry points
#include <hip/hip_runtime.h>
#include <cstdio>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <stddef.h>
#include <string>
#include <vector>
#include <mutex>
#include <new>

#include "../../include/rovat.h"
#include "rv_dev_wave.h"
#include "rv_dev_env.h"
#include "rv_dev_obs.h"
#include "rv_dev_grasp_sampler.h"
#include "rv_dev_grasp_quality.h"
#include "rv_dev_grasp_refine.h"
#include "rv_dev_contacts.h"
#include "rv_dev_plan.h"
#include "rv_dev_cem.h"
#include "rv_dev_depth_noise.h"
#include "rv_dev_push_sampler.h"
#include "rv_dev_push_route.h"
#include "rv_dev_view.h"
#include "rv_dev_grasp_train.h"
#include "rv_dev_segment.h"
#include "rv_dev_ward.h"

using namespace rv;

#include "rv_env_kernel.h"
#include "rv_dev_state.h"

#define ENV_THREAD() const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return; DevEnv& e = envs[i];

__global__ void k_init(DevEnv* envs, int n, float mu_finger, float mu_table, const rv_config* cfg) {
  ENV_THREAD();
  uint32_t* p = reinterpret_cast<uint32_t*>(&e);
  for (int k = 0; k < (int)(sizeof(DevEnv) / 4); ++k) p[k] = 0u;
  for (int b = 0; b < RV_MAXB; ++b) e.body[b][6] = 1.0f;
  for (int f = 0; f < RV_NFRAME; ++f) e.fquat[f][3] = 1.0f;
  e.done = 1;  // RobotEnv.__init__: self._done = True (robot_env.py:66)
  e.mu_finger = mu_finger; e.mu_table = mu_table;
  camera_reset(e, cfg, 0, 0);      // (the unperturbed calibration until the first env.reset())
}
__global__ void k_get_body_state(const DevEnv* envs, int n, float* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  for (int b = 0; b < RV_MAXB; ++b) for (int k = 0; k < 13; ++k) out[((size_t)i * RV_MAXB + b) * 13 + k] = envs[i].body[b][k];
}
__global__ void k_set_body_state(DevEnv* envs, int n, const float* in) {
  ENV_THREAD();
  for (int b = 0; b < RV_MAXB; ++b) for (int k = 0; k < 13; ++k) e.body[b][k] = in[((size_t)i * RV_MAXB + b) * 13 + k];
  for (int m = 0; m < RV_NMAN; ++m) e.man[m].n = 0;
  for (int b = 0; b < RV_MAXB; ++b) { e.asleep[b] = 0; e.sleep_count[b] = 0; e.deact_count[b] = 0; e.still_count[b] = 0; e.undisturbed[b] = 0; }
}
__global__ void k_get_body_params(const DevEnv* envs, int n, float* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  const DevEnv& e = envs[i];
  for (int b = 0; b < RV_MAXB; ++b) {
    float* o = out + ((size_t)i * RV_MAXB + b) * 8;
    o[0] = (float)e.active[b]; o[1] = (float)e.shape[b]; o[2] = e.scale[b]; o[3] = e.mass[b]; o[4] = e.friction[b];
    o[5] = (float)e.frozen[b]; o[6] = e.table_z; o[7] = (float)e.asleep[b];
  }
}
__global__ void k_set_body_params(DevEnv* envs, int n, const float* in, const rv_config* cfg, const rv_scene* scene) {
  ENV_THREAD();
  Consts K; K.cfg = cfg; K.arm = &scene->arm; K.scene = scene; K.stop_after = 0;
  int nb = 0;
  for (int b = 0; b < RV_MAXB; ++b) {
    const float* o = in + ((size_t)i * RV_MAXB + b) * 8;
    e.active[b] = (int)o[0]; e.shape[b] = (int)o[1]; e.scale[b] = o[2]; e.friction[b] = o[4]; e.frozen[b] = (int)o[5]; e.asleep[b] = 0; e.sleep_count[b] = 0; e.deact_count[b] = 0; e.still_count[b] = 0; e.undisturbed[b] = 0;
    if (b == 0) e.table_z = o[6];
    if (e.active[b]) { body_set_mass(e, K, b, o[3]); nb++; }
  }
  e.n_bodies = nb;
}
__global__ void k_get_joint_state(const DevEnv* envs, int n, float* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  for (int j = 0; j < RV_NJ; ++j) { out[((size_t)i * RV_NJ + j) * 2] = envs[i].q[j]; out[((size_t)i * RV_NJ + j) * 2 + 1] = envs[i].qd[j]; }
}
__device__ void update_link_frames(DevEnv& e, const rv_arm* a) {
  LimbFK F;
  fk_limb(a, e.q, F, nullptr);
  for (int f = 0; f <= RV_NLIMB; ++f) { st3(e.fpos[f], F.pos[f]); stq(e.fquat[f], F.quat[f]); }
  m3 r7 = qmat(F.quat[7]);
  v3 yax = mk(r7.m[1], r7.m[4], r7.m[7]);
  for (int k = 0; k < 2; ++k) {
    st3(e.fpos[8 + k], madd(F.pos[7], yax, a->finger_y0[k] + e.q[7 + k]));
    stq(e.fquat[8 + k], F.quat[7]);
  }
}
__global__ void k_set_joint_state(DevEnv* envs, int n, const float* in, const rv_config* cfg, const rv_scene* scene) {
  ENV_THREAD();
  const rv_arm* a = &scene->arm;
  for (int j = 0; j < RV_NJ; ++j) { e.q[j] = in[((size_t)i * RV_NJ + j) * 2]; e.qd[j] = in[((size_t)i * RV_NJ + j) * 2 + 1]; e.motor_q[j] = e.q[j]; }
  if (!e.arm_enabled) {
    for (int j = 0; j < RV_NJ; ++j) { e.motor_on[j] = 0; e.motor_kp[j] = cfg->kp; e.motor_kd[j] = cfg->kd; e.vmax_cmd[j] = a->v_max[j]; }
    arm_reset_targets(e); e.gripper_ready_time = 0.0f; e.arm_enabled = 1;
  }
  update_link_frames(e, a);
}
__global__ void k_get_link_poses(const DevEnv* envs, int n, float* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  for (int f = 0; f < RV_NFRAME; ++f) {
    float* o = out + ((size_t)i * RV_NFRAME + f) * 7;
    for (int k = 0; k < 3; ++k) o[k] = envs[i].fpos[f][k];
    for (int k = 0; k < 4; ++k) o[3 + k] = envs[i].fquat[f][k];
  }
}
#ifdef RV_PROFILE
__global__ void k_debug_profile(const DevEnv* envs, int n, unsigned long long* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) for (int k = 0; k < 48; ++k) out[(size_t)i * 48 + k] = envs[i].prof[k];
}
#endif
__global__ void k_get_env_counters(const DevEnv* envs, int n, int32_t* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  const DevEnv& e = envs[i]; int32_t* o = out + (size_t)i * RV_NCOUNTERS;
  o[8] = e.awake_last; o[9] = e.pairs_last;
  o[0] = e.sim_steps; o[1] = e.num_steps; o[2] = e.num_episodes; o[3] = e.phase; o[4] = e.done; o[5] = e.is_safe; o[6] = e.is_effective; o[7] = e.substeps_last;
}
__global__ void k_set_actions(DevEnv* envs, int n, const float* a, int G) {
  ENV_THREAD();
  for (int g = 0; g < G; ++g) for (int k = 0; k < 4; ++k) e.action[g][k] = a[((size_t)i * G + g) * 4 + k];
}
// rv_step_begin: the next action of the flagged envs; they are stepping from now on
__global__ void k_step_begin(DevEnv* envs, int n, const float* actions, const uint8_t* mask, int G) {
  ENV_THREAD();
  if (mask && !mask[i]) return;
  if (e.in_step == 1) return;                     // (still in the middle of its step: the action is ignored)
  for (int g2 = 0; g2 < G; ++g2) for (int k = 0; k < 4; ++k) e.action[g2][k] = actions[((size_t)i * G + g2) * 4 + k];
  e.in_step = e.done ? 2 : 1;
  e.step_stage = -1;
}
__global__ void k_reset_targets(DevEnv* envs, int n) {
  ENV_THREAD();
  arm_reset_targets(e);   // ControllableBody.reset_targets (controllable_body.py:347-350)
}
__global__ void k_set_int(int* p, int v) { *p = v; }
// BulletPhysics.position_control_array (bullet_physics.py:1061-1104): POSITION_CONTROL
// motor targets for the joints whose mask byte is set
__global__ void k_set_motor_targets(DevEnv* envs, int n, const float* q, const uint8_t* mask, const rv_config* cfg) {
  ENV_THREAD();
  for (int j = 0; j < RV_NJ; ++j) {
    if (mask && !mask[(size_t)i * RV_NJ + j]) continue;
    e.motor_on[j] = 1; e.motor_q[j] = q[(size_t)i * RV_NJ + j]; e.motor_kp[j] = cfg->kp; e.motor_kd[j] = cfg->kd;
  }
}
struct ConArgs { int body, child, type; float lp[3], lq[4], tp[3], tq[4], fmax; };
__global__ void k_set_constraint(DevEnv* envs, int n, ConArgs a) {
  ENV_THREAD();
  const int b = a.body;
  // (a body that went to sleep hanging from its constraint must notice that it changed or is gone)
  if (a.fmax < 0.0f) e.con_on[b] = 0;
  else {
    e.con_on[b] = a.type | ((a.child + 1) << 4); e.con_fmax[b] = a.fmax;      // (RV_CON_TYPE / RV_CON_CHILD, rv_dev_env.h)
    for (int k = 0; k < 3; ++k) { e.con_lpos[b][k] = a.lp[k]; e.con_tpos[b][k] = a.tp[k]; }
    for (int k = 0; k < 4; ++k) { e.con_lquat[b][k] = a.lq[k]; e.con_tquat[b][k] = a.tq[k]; }
  }
  e.asleep[b] = 0; e.sleep_count[b] = 0; e.deact_count[b] = 0; e.still_count[b] = 0; e.undisturbed[b] = 0;
  if (a.child >= 0 && a.child < RV_MAXB) { const int cb = a.child; e.asleep[cb] = 0; e.sleep_count[cb] = 0; e.deact_count[cb] = 0; e.still_count[cb] = 0; e.undisturbed[cb] = 0; }
}
__global__ void k_set_friction(DevEnv* envs, int n, float mu_finger, float mu_table) {
  ENV_THREAD();
  if (mu_finger >= 0.0f) e.mu_finger = mu_finger;
  if (mu_table >= 0.0f) e.mu_table = mu_table;
}
__global__ void k_grip(DevEnv* envs, int n, float value, const rv_config* cfg, const rv_scene* scene) {
  ENV_THREAD();
  grip_env(e, &scene->arm, cfg, value);
}
__global__ void k_set_joint_targets(DevEnv* envs, int n, const float* q, const rv_config* cfg, const rv_scene* scene, float timeout, float threshold) {
  ENV_THREAD();
  // SawyerSim.move_to_joint_positions (sawyer_sim.py:186-234)
  arm_reset_targets(e);
  for (int j = 0; j < RV_NLIMB; ++j) e.vmax_cmd[j] = cfg->limb_max_velocity_ratio * scene->arm.v_max[j];
  JTarget& t = e.jt;
  t.active = 1; t.n_idx = RV_NLIMB; t.has_vel = 1; t.from_ik = 0;
  for (int j = 0; j < RV_NLIMB; ++j) { t.idx[j] = j; t.pos[j] = q[(size_t)i * RV_NLIMB + j]; }
  t.start_t = cfg->dt * (float)e.sim_steps; t.stop_t = t.start_t + (timeout > 0.0f ? timeout : cfg->limb_timeout); t.has_stop = 1;
  t.pos_thr = threshold > 0.0f ? threshold : cfg->limb_position_threshold; t.vel_thr = cfg->velocity_threshold;
}
__global__ void k_set_link_target(DevEnv* envs, int n, const float* pose, const rv_config* cfg, const rv_scene* scene, float timeout, float threshold) {
  ENV_THREAD();
  // SawyerSim.move_to_gripper_pose (sawyer_sim.py:236-308)
  arm_reset_targets(e);
  for (int j = 0; j < RV_NLIMB; ++j) e.vmax_cmd[j] = cfg->limb_max_velocity_ratio * scene->arm.v_max[j];
  LTarget& t = e.lt;
  t.active = 1; t.has_pose = 1; t.nq = 0;
  for (int k = 0; k < 7; ++k) t.pose[k] = pose[(size_t)i * 7 + k];
  t.start_t = cfg->dt * (float)e.sim_steps; t.stop_t = t.start_t + (timeout > 0.0f ? timeout : cfg->limb_timeout); t.has_stop = 1;
  t.pos_thr = threshold > 0.0f ? threshold : cfg->limb_position_threshold; t.vel_thr = cfg->velocity_threshold;
}
__global__ void k_set_link_path(DevEnv* envs, int n, const float* poses, int n_poses, const rv_config* cfg, const rv_scene* scene, float timeout, float threshold) {
  ENV_THREAD();
  // SawyerSim.move_along_gripper_path (sawyer_sim.py:310-360) -> ControllableBody.set_target_link_poses
  // (controllable_body.py:322-345): the poses are queued, the first one becomes the link target
  arm_reset_targets(e);
  for (int j = 0; j < RV_NLIMB; ++j) e.vmax_cmd[j] = cfg->limb_max_velocity_ratio * scene->arm.v_max[j];
  LTarget& t = e.lt;
  t.active = 1; t.has_pose = 0; t.nq = n_poses;
  for (int q = 0; q < n_poses; ++q) for (int k = 0; k < 7; ++k) t.queue[q][k] = poses[((size_t)i * n_poses + q) * 7 + k];
  t.start_t = cfg->dt * (float)e.sim_steps; t.stop_t = t.start_t + (timeout > 0.0f ? timeout : cfg->limb_timeout); t.has_stop = 1;
  t.pos_thr = threshold > 0.0f ? threshold : cfg->limb_position_threshold; t.vel_thr = cfg->velocity_threshold;
  lt_pop(t);
}
__global__ void k_set_max_joint_velocities(DevEnv* envs, int n, const float* v) {
  ENV_THREAD();
  // ControllableBody.set_max_joint_velocities (controllable_body.py:357-372): the speed limits of the limb joints that the
  // running (and the next) targets are followed with -- SawyerSim.move_to_*(speed=...) sends them with every motion command
  // (sawyer_sim.py:212-220, 285-293, 336-344); a target setter puts LIMB_MAX_VELOCITY_RATIO x the URDF limits back
  for (int j = 0; j < RV_NLIMB; ++j) e.vmax_cmd[j] = v[(size_t)i * RV_NLIMB + j];
}
__global__ void k_robot_ready(DevEnv* envs, int n, uint8_t* out, const rv_config* cfg) {
  ENV_THREAD();
  // SawyerSim.is_limb_ready -> ControllableBody.is_ready(limb joints) (sawyer_sim.py:394-400, controllable_body.py:565-595):
  // like the reference's, the query retires targets that are done (reached, timed out, path exhausted)
  const float now = cfg->dt * (float)e.sim_steps;
  {
    const LTarget& t = e.lt;
    if (!t.has_stop || now >= t.stop_t || (!t.has_pose && t.nq == 0)) lt_reset(e.lt);
  }
  {
    const JTarget& t = e.jt;
    if (!t.has_stop || now >= t.stop_t || check_joints_reached(e)) jt_reset(e.jt);
  }
  int ready = 1;
  if (e.lt.active) ready = 0;                 // (every limb joint index < end-effector link index)
  if (e.jt.active) for (int k = 0; k < e.jt.n_idx; ++k) if (e.jt.idx[k] < RV_NLIMB) ready = 0;
  out[(size_t)i * 2] = (uint8_t)ready;
  // SawyerSim.is_gripper_ready (sawyer_sim.py:402-408): 0.5 s of simulated time after the last grip command
  out[(size_t)i * 2 + 1] = (uint8_t)(now >= e.gripper_ready_time);
}
__global__ void k_compute_ik(const DevEnv* envs, int n, const float* pose, float* q, const rv_config* cfg, const rv_scene* scene) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  Consts K; K.cfg = cfg; K.arm = &scene->arm; K.scene = scene; K.stop_after = 0;
  float p[7], q0[RV_NLIMB], out[RV_NLIMB];
  for (int k = 0; k < 7; ++k) p[k] = pose[(size_t)i * 7 + k];
  for (int j = 0; j < RV_NLIMB; ++j) q0[j] = envs[i].q[j];
  arm_ik(K, q0, p, out);
  for (int j = 0; j < RV_NLIMB; ++j) q[(size_t)i * RV_NLIMB + j] = out[j];
}
__global__ void k_query_contacts(const DevEnv* envs, int n, uint8_t* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  const DevEnv& e = envs[i]; uint8_t* o = out + (size_t)i * (2 + RV_MAXB);
  o[0] = (uint8_t)e.flag_arm_table; o[1] = (uint8_t)arm_touches_movables(e);
  for (int b = 0; b < RV_MAXB; ++b) o[2 + b] = (uint8_t)(e.active[b] && e.flag_arm_body[b]);      // (a static body: never)
}
__global__ void k_get_camera(const DevEnv* envs, int n, float* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  const DevEnv& e = envs[i]; float* o = out + (size_t)i * 17;
  for (int k = 0; k < 5; ++k) o[k] = e.cam_intrinsics[k];
  for (int k = 0; k < 9; ++k) o[5 + k] = e.cam_rotation[k];
  for (int k = 0; k < 3; ++k) o[14 + k] = e.cam_translation[k];
}
__global__ void k_manifold_counts(const DevEnv* envs, int n, int32_t* out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  for (int m = 0; m < RV_NMAN; ++m) out[(size_t)i * RV_NMAN + m] = envs[i].man[m].n;
}
__global__ void k_observe(const DevEnv* envs, int n, rv_obs_buffers o, const rv_config* cfg) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  obs_write_row(&envs[i], o, (size_t)i, cfg);
}
__global__ void k_obs_snap(const DevEnv* envs, int n, ObsSnap* snaps, const rv_scene* scene) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  obs_snap_fill(envs[i], &scene->arm, snaps[i]);
}
// SegmentedPointCloudObs (camera_obs.py:182-238): one wave per (observation, body); see rv_dev_obs.h
__global__ __launch_bounds__(64) void k_point_cloud(const ObsSnap* snaps, int n_snaps, int n_envs, float* out,
                                                    const rv_config* c, const rv_scene* scene) {
  __shared__ uint32_t s_pix[RV_PC_MAXPIX];
  __shared__ float s_dep[RV_PC_MAXPIX];
  __shared__ uint32_t s_key[RV_PC_MAXPIX];
  __shared__ float s_rot[RV_MAXB][9];
  const int si = (int)blockIdx.x / RV_MAXB, b = (int)blockIdx.x % RV_MAXB;
  if (si >= n_snaps) return;
  point_cloud_render(snaps[si], b, out + ((size_t)si * RV_MAXB + b) * (size_t)c->num_points * 3, (uint32_t)(c->env_id_offset + si % n_envs),
                     c, scene, s_pix, s_dep, s_key, s_rot);
}
// ... behind a recorded rollout whose finished workgroups have rendered already (rv_env_kernel.h, "the tail"): rendered[si] = 1
// marks their rows, whose blocks return at once; n_residual counts the rows rendered here.  (A kernel of its own: with the
// flag test in it k_point_cloud compiled to other, slower code -- configs 3 and 5 spend 45 - 75 ms in that kernel.)
__global__ __launch_bounds__(64) void k_point_cloud_rest(const ObsSnap* snaps, int n_snaps, int n_envs, float* out,
                                                         const rv_config* c, const rv_scene* scene, const uint8_t* rendered, int* n_residual) {
  __shared__ uint32_t s_pix[RV_PC_MAXPIX];
  __shared__ float s_dep[RV_PC_MAXPIX];
  __shared__ uint32_t s_key[RV_PC_MAXPIX];
  __shared__ float s_rot[RV_MAXB][9];
  const int si = (int)blockIdx.x / RV_MAXB, b = (int)blockIdx.x % RV_MAXB;
  if (si >= n_snaps) return;
  if (rendered[si]) return;
  if (b == 0 && threadIdx.x == 0) atomicAdd(n_residual, 1);
  point_cloud_render(snaps[si], b, out + ((size_t)si * RV_MAXB + b) * (size_t)c->num_points * 3, (uint32_t)(c->env_id_offset + si % n_envs),
                     c, scene, s_pix, s_dep, s_key, s_rot);
}
// CameraObs 'depth' / 'segmask' (camera_obs.py:33-88 over BulletCamera._frames,
// bullet_camera.py:188-235): the same ray cast as the point cloud, one thread per pixel.
// depth: eye z, 0 where nothing is hit; segmask: body index, RV_MAXB = table, RV_MAXB + 1 = arm, 255 = nothing
__global__ void k_render(const ObsSnap* snaps, int n, float* depth, uint8_t* seg, const rv_config* c, const rv_scene* scene) {
  const int H = c->cam_height, W = c->cam_width;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * H * W) return;
  const int i = (int)(t / ((size_t)H * W)); const int px = (int)(t % ((size_t)H * W));
  const int v = px / W, u = px - v * W;
  const ObsSnap& s = snaps[i];
  float rot[RV_MAXB][9];
  for (int b = 0; b < RV_MAXB; ++b) { m3 m = qmat(ldq(s.pose[b] + 3)); stm(rot[b], m); }
  const v3 cam_o = cam_position(&s);
  float d;
  int who = render_pixel(c, scene, s, rot, cam_o, cam_to_world_dir(&s, pixel_dir_cam(&s, (float)u, (float)v)), &d);
  if (who >= 0 && !(d > c->cam_near)) who = -1;
  if (depth) depth[t] = who >= 0 ? d : 0.0f;
  if (seg) seg[t] = who >= 0 ? (uint8_t)who : (uint8_t)255;
}
__global__ void k_reward(const DevEnv* envs, int n, float* reward, uint8_t* done) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  // an env whose episode is over is not stepped by rv_step_macro (the reference raises
  // "Forget to reset?", robot_env.py:244-245): it reports reward 0, done
  if (reward) reward[i] = envs[i].reward_valid ? envs[i].last_reward : 0.0f;
  if (done) done[i] = (uint8_t)envs[i].done;
}
__global__ void k_returns(const DevEnv* envs, int n, float* r) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  r[i] = envs[i].episode_reward;
}
__global__ void k_policy_random(int n, const rv_config* cfg, int macro_index, float* actions) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  int G = cfg->num_goal_steps > 0 ? cfg->num_goal_steps : 1;
  random_action(cfg, cfg->env_id_offset + i, macro_index, actions + (size_t)i * G * 4);
}
// HeuristicPushSampler._sample (heuristic_push_sampler.py:66-123): one wave
// per env, 64 candidate pushes per round; the lowest successful attempt wins.
__global__ __launch_bounds__(64) void k_policy_heuristic(const DevEnv* envs, int n, const rv_config* c, int max_attempts, float* actions) {
  const int i = (int)blockIdx.x; if (i >= n) return;
  const int lane = (int)threadIdx.x;
  const DevEnv& e = envs[i];
  int G = c->num_goal_steps > 0 ? c->num_goal_steps : 1;
  int nb = 0;
  for (int b = 0; b < RV_MAXB; ++b) nb += body_movable(e, b);
  if (nb == 0) nb = 1;
  // the policy reads the counters from the observation (push_policy.py:46-49), i.e. the
  // env.attributes snapshot; like the reference it assumes the first nb slots are the bodies
  // (heuristic_push_sampler.py:70: position[:num_bodies])
  const int n_ep = e.obs_num_episodes, n_st = e.obs_num_steps;
  int body_id = n_ep % nb;
  float base = (float)n_ep * 42.0f;
  base = base - 2.0f * RV_PI * ffloorr(base / (2.0f * RV_PI));
  float lo0 = c->cspace_low[0], hi0 = c->cspace_high[0], lo1 = c->cspace_low[1], hi1 = c->cspace_high[1];
  float s0 = 0.0f, s1 = 0.0f, m0 = 0.0f, m1 = 0.0f;
  int found_att = -1;
  for (int base_att = 0; base_att < max_attempts; base_att += 64) {
    int att = base_att + lane;
    bool good = false;
    if (att < max_attempts) {
      Rng g = rng_init(c->seed_lo, c->seed_hi, (uint32_t)(c->env_id_offset + i), RV_STREAM_HEUR, (uint32_t)(n_ep * 64 + n_st));
      g.c0 = (uint32_t)att * 2u;
      s0 = rng_uniform(g, -1.0f, 1.0f); s1 = rng_uniform(g, -1.0f, 1.0f);
      float ang = base + rng_uniform(g, -0.25f * RV_PI, 0.25f * RV_PI);
      float sn, co; sincosr(ang, &sn, &co);
      m0 = fclampr(co + rng_uniform(g, -0.3f, 0.3f), -1.0f, 1.0f);
      m1 = fclampr(sn + rng_uniform(g, -0.3f, 0.3f), -1.0f, 1.0f);
      float x = s0 * (0.5f * (hi0 - lo0)) + 0.5f * (hi0 + lo0);
      float y = s1 * (0.5f * (hi1 - lo1)) + 0.5f * (hi1 + lo1);
      float ex = fclampr(x + m0 * c->translation_x, lo0, hi0);
      float ey = fclampr(y + m1 * c->translation_y, lo1, hi1);
      int safe = 1;
      for (int b = 0; b < nb; ++b) {
        float dx = e.obs_pos[b][0] - x, dy = e.obs_pos[b][1] - y;
        if (!(fsqrtr(dx * dx + dy * dy) > 0.05f)) safe = 0;
      }
      float dx1 = e.obs_pos[body_id][0] - x, dy1 = e.obs_pos[body_id][1] - y;
      float dx2 = e.obs_pos[body_id][0] - ex, dy2 = e.obs_pos[body_id][1] - ey;
      int clear = fsqrtr(dx1 * dx1 + dy1 * dy1) >= 0.01f && fsqrtr(dx2 * dx2 + dy2 * dy2) >= 0.01f;
      good = safe && !clear;
    }
    unsigned long long ballot = __ballot(good);
    if (ballot) { found_att = base_att + (int)__ffsll((long long)ballot) - 1; break; }
  }
  // winner (or, like the reference, the last attempt drawn) writes the action
  int writer = found_att >= 0 ? (found_att & 63) : ((max_attempts - 1) & 63);
  if (lane == writer) {
    for (int g2 = 0; g2 < G; ++g2) {
      float* a = actions + ((size_t)i * G + g2) * 4;
      a[0] = s0; a[1] = s1; a[2] = m0; a[3] = m1;
    }
  }
}
__global__ void k_stats(const DevEnv* envs, int n, rv_macro_stats* st, float success_thresh) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); if (i >= n) return;
  const DevEnv& e = envs[i];
  typedef unsigned long long u64;
  if (e.substeps_last > 0) {
    atomicAdd((u64*)&st->substeps, (u64)e.substeps_last);
    atomicMax((u64*)&st->max_substeps, (u64)e.substeps_last);
    atomicAdd((u64*)&st->awake_substeps, (u64)e.awake_last);
  }
  if (e.stepped) {
    atomicAdd((u64*)&st->env_steps, (u64)e.stepped);
    // per-launch sums kept by env_step (a rollout launch takes several steps per env)
    if (e.l_unsafe) atomicAdd((u64*)&st->unsafe, (u64)e.l_unsafe);
    if (e.l_ineffective) atomicAdd((u64*)&st->ineffective, (u64)e.l_ineffective);
    if (e.l_useful) atomicAdd((u64*)&st->useful, (u64)e.l_useful);
    if (e.l_episodes) atomicAdd((u64*)&st->episodes_done, (u64)e.l_episodes);
    if (e.l_successes) atomicAdd((u64*)&st->successes, (u64)e.l_successes);
  }
}

__global__ void k_render_rgb(const ObsSnap* snaps, int n, uint8_t* rgb, const rv_config* c, const rv_scene* scene) {
  const int H = c->cam_height, W = c->cam_width;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * H * W) return;
  const int i = (int)(t / ((size_t)H * W)); const int px = (int)(t % ((size_t)H * W));
  const int v = px / W, u = px - v * W;
  const ObsSnap& s = snaps[i];
  float rot[RV_MAXB][9];
  for (int b = 0; b < RV_MAXB; ++b) { m3 m = qmat(ldq(s.pose[b] + 3)); stm(rot[b], m); }
  const v3 cam_o = cam_position(&s);
  float d; v3 nrm;
  int who = render_pixel(c, scene, s, rot, cam_o, cam_to_world_dir(&s, pixel_dir_cam(&s, (float)u, (float)v)), &d, &nrm);
  if (who >= 0 && !(d > c->cam_near)) who = -1;
  shade_rgb(who, nrm, rgb + t * 3);
}

// ------------------------------------------------------------------ host ABI
struct rv_world {
  rv_config cfg;
  int device;
  int n;
  hipStream_t stream;
  rv_config* d_cfg;
  rv_scene* d_scene;
  DevEnv* d_envs;
  rv_macro_stats* d_stats;
  int* d_budget;
  ObsSnap* d_snaps; size_t n_snaps_cap;   // pose snapshots for the point-cloud render
  // the words of the rollout kernel's tail (rv_env_kernel.h, rv_pc_tail; grown on demand, zeroed before every launch that
  // uses them): [2] rows rendered by the tail / by the launch after it, [N] done, [N] claimed, then [n_steps x N] rendered
  // bytes.  pc_rows: snapshot rows of the last recorded rollout (0: it took no point clouds), pc_flags: it used the words
  int* d_pc_tail; size_t pc_tail_cap; size_t pc_rows; bool pc_flags;
  hipEvent_t ev0, ev1;
  bool timed;
  int auto_reset;                         // rv_set_auto_reset
  int occ2;                               // more envs than SIMDs: launch k_env_occ2 (rv_env_kernel.h)
  // rollouts of a world with more envs than the GPU has wave slots go through task queues, one per XCD (rv_env_kernel.h):
  // q_grid workgroups (what is resident at a time), d_q = [RV_Q_CTL_WORDS control words][RV_Q_NQ rings of q_ring slots];
  // q_launch numbers the queued launches, q_used: a queued launch ran since rv_get_stats last looked at its error word
  int q_grid; int* d_q; size_t q_cap; int q_launch; bool q_used;
  // rv_policy_antipodal: the depth it renders itself, the per-env filter scratch (floats; grown on demand)
  float* d_ap_depth; size_t ap_depth_cap; float* d_ap_scratch; size_t ap_scratch_cap;
  // rv_branch / rv_plan_simulate: FNV-1a of the rv_scene the world was made from (two worlds may exchange env blocks only
  // when they share it), and the event that orders a copy between the streams of two worlds
  uint64_t scene_hash; hipEvent_t ev_state;
  // rv_depth_noise: [N] multipliers, [N] flags (as words), then the noise grid when the caller gives none (floats; grown
  // on demand)
  float* d_dn_scratch; size_t dn_scratch_cap;
  // rv_get_route_field / rv_policy_route_multi: D[64] and walkable[64] of the config's tiles (rv_dev_push_route.h), made at
  // first use -- no setter changes the tile fields of cfg after rv_create
  uint8_t* d_route;
  // rv_render_view: [V] env indices then [V][17] camera rows, on the device and in pinned host memory (what was uploaded
  // last: an identical call skips the copy); ev_view: the last upload has left the pinned copy
  uint8_t* d_view; uint8_t* h_view; size_t view_cap, view_bytes; hipEvent_t ev_view;
  // rv_segment_cloud: [env_count][M] rank -> point index (words; grown on demand)
  float* d_seg_scratch; size_t seg_scratch_cap;
};

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(RV_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
#define WCHK(w) do { if (!(w)) return fail(RV_ERR_VALUE, "null world"); HIPCHK(hipSetDevice((w)->device)); } while (0)

static inline dim3 grid1(int n) { return dim3((unsigned)((n + 127) / 128)); }
#define TPB 128

// the register-rich kernel while every env has a SIMD of its own, the two-waves-per-SIMD build beyond that
static void launch_k_env(rv_world* w, int mode, const EnvKernelArgs& a) {
  const int n_grid = a.q_slots ? w->q_grid : w->n;
  if (w->occ2) rv_launch_k_env_occ2(mode, a, n_grid, w->stream);
  else rv_launch_k_env_here(mode, a, n_grid, w->stream);
}
#define RV_QUEUE_MIN_STEPS 10
__global__ void k_queue_init(int* q, long long words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < words) q[i] = i < RV_Q_CTL_WORDS ? 0 : -1;      // counters 0 (the error word too), every slot "not yet published"
}
// MODE_ROLLOUT of n_steps through the task queues?  Worlds with more envs than resident workgroups (RV_QUEUE=0: never)
// pool > 0: the work-conserving rollout (rv_rollout_async) -- `pool` tasks in all, an env goes back to the tail after every
// step, so the envs take turns and one in a slow state simply gets fewer of them
// (`a` arrives with the queues off: launch_env)
static int queue_setup(rv_world* w, int n_steps, EnvKernelArgs& a, long long pool = 0) {
  const char* q = getenv("RV_QUEUE");      // (read per launch: the tests compare the two schedules in one process)
  // (measured with the per-XCD queues and the keep rule of k_env, profiles/r06_queue_variants.txt -- 8192 envs: 20 steps + 14 %, 10 steps
  // + 13 ... 16 %, 5 steps + 16 ... 19 %, 2 steps - 5 %; 4096 concave envs x 10 steps, bound by their slowest env: + - 0;
  // 8192 envs without deactivation, 8 steps, bound by envs that get slower step after step: - 6 %.  Rollouts of 10 steps and
  // more (RV_QUEUE_MIN_STEPS) go through the queues.  RV_QUEUE=1 forces them, 0 forbids them)
  if ((q && atoi(q) == 0) || w->q_grid <= 0 || w->n <= w->q_grid || (pool == 0 && n_steps < RV_QUEUE_MIN_STEPS && !(q && atoi(q) == 1))) return RV_OK;
  const size_t total = pool > 0 ? (size_t)pool : (size_t)w->n * (size_t)n_steps;      // tasks that are begun
  if (total > ((size_t)1 << 24)) return RV_OK;      // (8 rings of `total` ints: 512 MB at most)
  // a ring holds what ONE XCD may be handed in the worst case: every task of the launch (an env is published once per
  // step it has left; in a pool once per task that was begun)
  const size_t ring = total;
  const size_t need = (size_t)RV_Q_CTL_WORDS + (size_t)RV_Q_NQ * ring;
  if (w->q_cap < need) {
    if (w->d_q) { HIPCHK(hipStreamSynchronize(w->stream)); HIPCHK(hipFree(w->d_q)); w->d_q = nullptr; w->q_cap = 0; }
    HIPCHK(hipMalloc(&w->d_q, need * sizeof(int)));
    w->q_cap = need;
  }
  if (w->q_used) {      // (the error word of the last queued launch, before it is zeroed)
    int err = 0;
    HIPCHK(hipMemcpyAsync(&err, w->d_q + RV_Q_ERR, sizeof(int), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    w->q_used = false;
    if (err) return fail(RV_ERR_STATE, "task queue: a block arrived with the wrong step / launch number, or a ring overflowed (code " + std::to_string(err) + ") in the previous queued launch");
  }
  a.q_ctl = w->d_q; a.q_slots = w->d_q + RV_Q_CTL_WORDS; a.q_cap = (int)ring; a.q_total = (int)total; a.q_pool = pool > 0 ? 1 : 0;
  a.q_launch = ++w->q_launch;
  a.q_debug = getenv("RV_QUEUE_DEBUG") != nullptr;
  a.q_global = getenv("RV_QUEUE_GLOBAL") != nullptr;
  { const char* st = getenv("RV_QUEUE_STICKY"); a.q_sticky = st ? atoi(st) : 1; }
  { const char* wt = getenv("RV_QUEUE_WT"); a.q_wt = wt ? atoi(wt) : 1; }      // (measurement aid: 0 = plain stores / loads of the block)
  { const char* sl = getenv("RV_QUEUE_STEAL"); a.q_steal = (sl ? atoi(sl) : 0) && a.q_wt; }      // (off: measured, no gain -- rv_env_kernel.h)
  hipLaunchKernelGGL(k_queue_init, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, w->stream, w->d_q, (long long)need);
  HIPCHK(hipGetLastError());
  w->q_used = true;
  return RV_OK;
}
// RV_POISON_LDS builds (tools/build_poison.py): which words of the scratch block start as garbage; everything by default
static void poison_range(EnvKernelArgs& a) {
  const char* lo = getenv("RV_POISON_LO"); const char* hi = getenv("RV_POISON_HI");
  a.poison_lo = lo ? atoi(lo) : 0; a.poison_hi = hi ? atoi(hi) : 0x7fffffff;
}
// The tail of a recorded rollout (rv_env_kernel.h, rv_pc_tail): finished workgroups of the plain launch of the
// register-rich kernel render point clouds; the k_point_cloud launch that follows renders the rows they left.
// count[0] / count[1]: rows rendered by the tail / by that launch (rv_last_tail_renders)
struct PcTail { int* count; int* done; int* claimed; uint8_t* rendered; float* out; int cap; };
// RV_PC_TAIL (read per launch, as RV_QUEUE): 0 = off, the clouds are all rendered after the kernel; unset or 1 = on.
// RV_PC_TAIL_CAP = n (a test aid that forces the mix): a finished workgroup renders n rows at most; 0 leaves every row
// to the launch after the kernel.  Worlds on the two-waves-per-SIMD build have no tail
static bool pc_tail_wanted(const rv_world* w, int n_steps) {
  const char* t = getenv("RV_PC_TAIL");
  return !(t && atoi(t) == 0) && !w->occ2 && n_steps < (1 << 24);
}
// the words of the tail for `rows` snapshot rows, zeroed on the world's stream
static int pc_tail_setup(rv_world* w, size_t rows, float* d_out, PcTail* t) {
  const size_t head = (size_t)(2 + 2 * (size_t)w->n) * sizeof(int), need = head + rows;
  if (w->pc_tail_cap < need) {
    if (w->d_pc_tail) { HIPCHK(hipStreamSynchronize(w->stream)); HIPCHK(hipFree(w->d_pc_tail)); w->d_pc_tail = nullptr; w->pc_tail_cap = 0; }
    HIPCHK(hipMalloc(&w->d_pc_tail, need));
    w->pc_tail_cap = need;
  }
  HIPCHK(hipMemsetAsync(w->d_pc_tail, 0, need, w->stream));
  t->count = w->d_pc_tail; t->done = w->d_pc_tail + 2; t->claimed = t->done + w->n;
  t->rendered = reinterpret_cast<uint8_t*>(w->d_pc_tail) + head; t->out = d_out;
  const char* cap = getenv("RV_PC_TAIL_CAP");
  t->cap = cap ? atoi(cap) : 0x7fffffff;
  if (t->cap < 0) t->cap = 0;
  return RV_OK;
}
template <int MODE>
static int launch_env(rv_world* w, const uint8_t* mask, int n_sub, float lin, float ang, int ca, int ms, int mx,
                      int first_index = 0, int auto_reset = 0, const RolloutRec* rec = nullptr,
                      int* budget = nullptr, int32_t* steps_taken = nullptr, long long pool_tasks = 0, const PcTail* tail = nullptr) {
  EnvKernelArgs a;
  a.budget = budget; a.steps_taken = steps_taken; a.budget_clk = 0; a.finished = nullptr;
  a.first_index = first_index; a.auto_reset = auto_reset;
  memset(&a.rec, 0, sizeof(a.rec));
  if (rec) a.rec = *rec;
  a.cfg = w->d_cfg; a.scene = w->d_scene; a.envs = w->d_envs; a.mask = mask; a.n_envs = w->n;
  { const char* ds = getenv("RV_DEBUG_STOP"); a.stop_after = ds ? atoi(ds) : 0; }
  a.n_substeps = n_sub; a.lin_thr = lin; a.ang_thr = ang; a.check_after = ca; a.min_stable = ms; a.max_steps = mx;
  a.q_slots = nullptr; a.q_ctl = nullptr; a.q_cap = 0; a.q_total = 0; a.q_pool = 0; a.q_launch = 0; a.q_wt = 0; a.q_sticky = 0; a.q_debug = 0; a.q_global = 0; a.q_steal = 0;
  poison_range(a);
  if (MODE == MODE_ROLLOUT && budget == nullptr) { int rc = queue_setup(w, n_sub, a); if (rc != RV_OK) return rc; }
  if (MODE == MODE_ROLLOUT && budget != nullptr && pool_tasks > 0) {
    // the work-conserving rollout of a world with more envs than resident workgroups: through the queue, or the
    // workgroups that are resident first would use the pool up before the others have started
    int rc = queue_setup(w, 0, a, pool_tasks); if (rc != RV_OK) return rc;
    if (a.q_slots) { a.budget = nullptr; a.n_substeps = 0x7fffffff; }      // (an env always has "steps left": the pool ends the launch)
  }
  a.pc_done = nullptr; a.pc_claimed = nullptr; a.pc_rendered = nullptr; a.pc_count = nullptr; a.pc_out = nullptr; a.pc_cap = 0;
  if (MODE == MODE_ROLLOUT && tail && a.q_slots == nullptr && !w->occ2 && a.rec.snaps) {      // (a queued launch has no tail: every row is left)
    a.pc_done = tail->done; a.pc_claimed = tail->claimed; a.pc_rendered = tail->rendered; a.pc_count = tail->count; a.pc_out = tail->out; a.pc_cap = tail->cap;
  }
  HIPCHK(hipMemsetAsync(w->d_stats, 0, sizeof(rv_macro_stats), w->stream));
  HIPCHK(hipEventRecord(w->ev0, w->stream));
  launch_k_env(w, MODE, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev1, w->stream));
  w->timed = true;
  hipLaunchKernelGGL(k_stats, grid1(w->n), dim3(TPB), 0, w->stream, w->d_envs, w->n, w->d_stats, w->cfg.success_thresh);
  HIPCHK(hipGetLastError());
  return RV_OK;
}

static int ensure_snaps(rv_world* w, size_t n) {
  if (w->n_snaps_cap >= n) return RV_OK;
  if (w->d_snaps) { HIPCHK(hipStreamSynchronize(w->stream)); HIPCHK(hipFree(w->d_snaps)); w->d_snaps = nullptr; w->n_snaps_cap = 0; }
  HIPCHK(hipMalloc(&w->d_snaps, sizeof(ObsSnap) * n));
  w->n_snaps_cap = n;
  return RV_OK;
}
// a lazily grown device buffer of `n` floats (as ensure_snaps)
static int ensure_floats(rv_world* w, float** buf, size_t* cap, size_t n) {
  if (*cap >= n) return RV_OK;
  if (*buf) { HIPCHK(hipStreamSynchronize(w->stream)); HIPCHK(hipFree(*buf)); *buf = nullptr; *cap = 0; }
  HIPCHK(hipMalloc(buf, sizeof(float) * n));
  *cap = n;
  return RV_OK;
}
// tail: the rows the rollout kernel's finished workgroups have rendered are flagged there and skipped here
static int launch_point_cloud(rv_world* w, size_t n_snaps, float* d_out, const PcTail* tail = nullptr) {
  if (tail) hipLaunchKernelGGL(k_point_cloud_rest, dim3((unsigned)(n_snaps * RV_MAXB)), dim3(64), 0, w->stream,
                               w->d_snaps, (int)n_snaps, w->n, d_out, w->d_cfg, w->d_scene, (const uint8_t*)tail->rendered, tail->count + 1);
  else hipLaunchKernelGGL(k_point_cloud, dim3((unsigned)(n_snaps * RV_MAXB)), dim3(64), 0, w->stream,
                          w->d_snaps, (int)n_snaps, w->n, d_out, w->d_cfg, w->d_scene);
  HIPCHK(hipGetLastError());
  return RV_OK;
}

// the checks rv_plan_reward and rv_plan_score share
static int plan_check(const rv_world* w, const rv_plan_params* p, const char* who) {
  if (!p) return fail(RV_ERR_VALUE, std::string(who) + ": null params");
  if (w->cfg.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, std::string(who) + ": a PushEnv world only");
  if (p->n_bodies < 1 || p->n_bodies > RV_MAXB) return fail(RV_ERR_VALUE, std::string(who) + ": n_bodies outside [1, RV_MAXB]");
  return RV_OK;
}
static bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// the kernel for B bodies; V4: the [4][2] records are read as two float4 (a 16-byte aligned base)
#define PLAN_DISPATCH(B, V4, F, ...) do { \
    switch (B) { \
      case 1: F<1, false>(__VA_ARGS__); break; \
      case 2: F<2, false>(__VA_ARGS__); break; \
      case 3: F<3, false>(__VA_ARGS__); break; \
      default: if (V4) F<4, true>(__VA_ARGS__); else F<4, false>(__VA_ARGS__); break; \
    } } while (0)
template <int B, bool V4>
static void launch_plan_reward(rv_world* w, const rv_plan_params& p, const float* s, const float* nx, long long m, float* r, uint8_t* t) {
  hipLaunchKernelGGL((k_plan_reward<B, V4>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, w->stream, w->d_cfg, p, s, nx, m, r, t);
}
template <int B, bool V4>
static void launch_plan_score(rv_world* w, const PlanArgs& a, int tpb) {
  hipLaunchKernelGGL((k_plan_score<B, V4>), dim3((unsigned)w->n), dim3((unsigned)tpb), 0, w->stream, w->d_envs, w->d_cfg, a);
}

// ---- env states as data (rv_dev_state.h)
static uint64_t bytes_hash(const void* p, size_t n) {      // FNV-1a
  const unsigned char* b = (const unsigned char*)p;
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
// block j of dst (n_dst blocks) takes block index[j] (NULL: j / s) of src (n_src blocks), on `st`.  16-byte accesses where
// the block size and both bases allow them.  (The grid's y extent ends at 65535: larger worlds take several launches.)
static int launch_gather(hipStream_t st, void* dst, const void* src, int n_dst, int n_src, const int32_t* index, int s) {
  const bool v4 = RV_STATE_VEC_OK && aligned_to(dst, 16) && aligned_to(src, 16);
  for (int j0 = 0; j0 < n_dst; j0 += 65535) {
    const int rows = n_dst - j0 < 65535 ? n_dst - j0 : 65535;
    if (v4) hipLaunchKernelGGL(k_env_blocks_gather<true>, dim3(1u, (unsigned)rows), dim3(RV_STATE_TPB), 0, st, (uint32_t*)dst, (const uint32_t*)src, j0, n_dst, n_src, index, s);
    else hipLaunchKernelGGL(k_env_blocks_gather<false>, dim3(1u, (unsigned)rows), dim3(RV_STATE_TPB), 0, st, (uint32_t*)dst, (const uint32_t*)src, j0, n_dst, n_src, index, s);
    HIPCHK(hipGetLastError());
  }
  return RV_OK;
}
// identity copies of whole worlds go through the runtime's device-to-device copy or through the gather kernel:
// RV_STATE_MEMCPY = 1 / 0 forces one (read per call: tools/state_branch_bench.py measures both in one process)
static bool state_identity_by_runtime() {
  const char* f = getenv("RV_STATE_MEMCPY");
  return f ? atoi(f) != 0 : RV_STATE_IDENTITY_BY_RUNTIME != 0;
}
// what rv_branch and rv_plan_simulate ask of their two worlds; nothing has been launched when this fails
static int branch_check(const rv_world* dst, const rv_world* src, int s, const char* who) {
  const std::string me(who);
  if (dst == src) return fail(RV_ERR_VALUE, me + ": the two worlds must differ");
  if (s < 1) return fail(RV_ERR_VALUE, me + ": s must be positive");
  if ((long long)dst->n != (long long)src->n * (long long)s) return fail(RV_ERR_VALUE, me + ": the destination needs n_envs = s x the source's n_envs");
  if (dst->device != src->device) return fail(RV_ERR_VALUE, me + ": the two worlds live on different devices");
  if (dst->scene_hash != src->scene_hash) return fail(RV_ERR_VALUE, me + ": the two worlds were made from different scenes");
  rv_config a = dst->cfg, b = src->cfg;
  a.n_envs = b.n_envs = 0; a.env_id_offset = b.env_id_offset = 0;
  if (memcmp(&a, &b, sizeof(rv_config)) != 0) return fail(RV_ERR_VALUE, me + ": the two worlds differ in more of rv_config than n_envs and env_id_offset");
  return RV_OK;
}
// env j of dst = env j / s of src.  dst's stream waits for what src's stream has been given so far; src's stream waits for
// the copy before it goes on (it may change the blocks next)
static int branch_copy(rv_world* dst, rv_world* src, int s) {
  const bool cross = dst->stream != src->stream;
  if (cross) { HIPCHK(hipEventRecord(dst->ev_state, src->stream)); HIPCHK(hipStreamWaitEvent(dst->stream, dst->ev_state, 0)); }
  int rc = launch_gather(dst->stream, dst->d_envs, src->d_envs, dst->n, src->n, nullptr, s); if (rc != RV_OK) return rc;
  if (cross) { HIPCHK(hipEventRecord(dst->ev_state, dst->stream)); HIPCHK(hipStreamWaitEvent(src->stream, dst->ev_state, 0)); }
  return RV_OK;
}

extern "C" {

const char* rv_last_error(void) { return g_err.c_str(); }

int rv_create(const rv_config* cfg, const rv_scene* scene, int device, rv_world** out) {
  if (!cfg || !scene || !out) return fail(RV_ERR_VALUE, "rv_create: null argument");
  if (cfg->n_envs <= 0) return fail(RV_ERR_VALUE, "rv_create: n_envs must be positive");
  if (cfg->n_bodies_max > RV_MAXB || cfg->n_bodies_min < 1 || cfg->n_bodies_min > cfg->n_bodies_max)
    return fail(RV_ERR_VALUE, "rv_create: body count outside [1, RV_MAXB]");
  if (scene->n_shapes <= 0 || scene->n_shapes > RV_MAX_SHAPES) return fail(RV_ERR_VALUE, "rv_create: bad n_shapes");
  if (cfg->wall_use && (cfg->n_bodies_max > RV_MAXB - 1 || cfg->wall_shape < 0 || cfg->wall_shape >= scene->n_shapes || !(cfg->wall_scale > 0.0f)))
    return fail(RV_ERR_VALUE, "rv_create: wall_use needs n_bodies_max <= RV_MAXB - 1, a shape template of the scene and a positive scale");
  int ndev = 0;
  hipError_t e0 = hipGetDeviceCount(&ndev);
  if (e0 != hipSuccess || ndev == 0)
    return fail(RV_ERR_HIP, "rv_create: no HIP device available (librovat_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(RV_ERR_VALUE, "rv_create: bad device index");
  HIPCHK(hipSetDevice(device));
  rv_world* w = new (std::nothrow) rv_world();
  if (!w) return fail(RV_ERR_STATE, "rv_create: out of host memory");
  w->cfg = *cfg; w->device = device; w->n = cfg->n_envs; w->stream = nullptr; w->timed = false;
  w->d_snaps = nullptr; w->n_snaps_cap = 0;
  w->d_pc_tail = nullptr; w->pc_tail_cap = 0; w->pc_rows = 0; w->pc_flags = false;
  w->d_ap_depth = nullptr; w->ap_depth_cap = 0; w->d_ap_scratch = nullptr; w->ap_scratch_cap = 0;
  w->d_dn_scratch = nullptr; w->dn_scratch_cap = 0;
  w->d_route = nullptr;
  w->d_view = nullptr; w->h_view = nullptr; w->view_cap = 0; w->view_bytes = 0;
  w->scene_hash = bytes_hash(scene, sizeof(rv_scene));
  {
    // one wave per env: with more envs than SIMDs the two-waves-per-SIMD build of the env kernel pays
    // (RV_ENV_OCC=1 / 2 in the environment forces a build: measurements)
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    w->occ2 = w->n > 4 * cus;
    w->q_grid = 0; w->d_q = nullptr; w->q_cap = 0; w->q_launch = 0; w->q_used = false;
    const char* f = getenv("RV_ENV_OCC");
    if (f && (f[0] == '1' || f[0] == '2')) w->occ2 = f[0] == '2';
    // the task queue's grid: every workgroup the GPU keeps resident of the kernel this world launches
    // (the occupancy query does not see the waves-per-SIMD cap of the build: one wave per SIMD at 512 registers, two at
    // 256 -- and the 20 KB LDS block allows eight workgroups per CU at most)
    int per_cu = w->occ2 ? rv_k_env_occ2_blocks_per_cu() : rv_k_env_blocks_per_cu_here();
    const int cap = w->occ2 ? 8 : 4;
    if (per_cu > cap) per_cu = cap;
    w->q_grid = per_cu > 0 ? per_cu * cus : 0;
  }
  HIPCHK(hipMalloc(&w->d_cfg, sizeof(rv_config)));
  HIPCHK(hipMalloc(&w->d_scene, sizeof(rv_scene)));
  HIPCHK(hipMalloc(&w->d_envs, sizeof(DevEnv) * (size_t)w->n));
  HIPCHK(hipMalloc(&w->d_stats, sizeof(rv_macro_stats)));
  HIPCHK(hipMalloc(&w->d_budget, sizeof(int)));
  HIPCHK(hipMemcpy(w->d_cfg, cfg, sizeof(rv_config), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(w->d_scene, scene, sizeof(rv_scene), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(w->d_stats, 0, sizeof(rv_macro_stats)));
  HIPCHK(hipEventCreate(&w->ev0));
  HIPCHK(hipEventCreate(&w->ev1));
  HIPCHK(hipEventCreateWithFlags(&w->ev_state, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&w->ev_view, hipEventDisableTiming));
  hipLaunchKernelGGL(k_init, grid1(w->n), dim3(TPB), 0, w->stream, w->d_envs, w->n, cfg->arm_friction, cfg->table_friction, w->d_cfg);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(w->stream));
  *out = w;
  return RV_OK;
}

int rv_destroy(rv_world* w) {
  if (!w) return RV_OK;
  (void)hipSetDevice(w->device);
  (void)hipStreamSynchronize(w->stream);
  (void)hipFree(w->d_cfg); (void)hipFree(w->d_scene);
  (void)hipFree(w->d_envs); (void)hipFree(w->d_stats); (void)hipFree(w->d_budget); if (w->d_q) (void)hipFree(w->d_q);
  if (w->d_snaps) (void)hipFree(w->d_snaps);
  if (w->d_pc_tail) (void)hipFree(w->d_pc_tail);
  if (w->d_ap_depth) (void)hipFree(w->d_ap_depth);
  if (w->d_ap_scratch) (void)hipFree(w->d_ap_scratch);
  if (w->d_dn_scratch) (void)hipFree(w->d_dn_scratch);
  if (w->d_route) (void)hipFree(w->d_route);
  if (w->d_view) (void)hipFree(w->d_view);
  if (w->d_seg_scratch) (void)hipFree(w->d_seg_scratch);
  if (w->h_view) (void)hipHostFree(w->h_view);
  (void)hipEventDestroy(w->ev0); (void)hipEventDestroy(w->ev1); (void)hipEventDestroy(w->ev_state); (void)hipEventDestroy(w->ev_view);
  delete w;
  return RV_OK;
}

int rv_set_stream(rv_world* w, void* s) { WCHK(w); w->stream = (hipStream_t)s; return RV_OK; }
int rv_synchronize(rv_world* w) { WCHK(w); HIPCHK(hipStreamSynchronize(w->stream)); return RV_OK; }
int rv_num_envs(const rv_world* w) { return w ? w->n : 0; }
int rv_env_kernel_build(const rv_world* w) { return !w ? 0 : w->occ2 ? RV_ENV_BUILD_OCC2 : RV_ENV_BUILD_OCC1; }

int rv_reset(rv_world* w, const uint8_t* d_env_mask) { WCHK(w); return launch_env<MODE_RESET>(w, d_env_mask, 0, 0, 0, 0, 0, 0); }
int rv_step_macro(rv_world* w) { WCHK(w); return launch_env<MODE_MACRO>(w, nullptr, 0, 0, 0, 0, 0, 0); }
int rv_rollout(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset, float* d_rewards, uint8_t* d_dones) {
  WCHK(w);
  if (n_steps <= 0) return fail(RV_ERR_VALUE, "rv_rollout: n_steps must be positive");
  RolloutRec rec; memset(&rec, 0, sizeof(rec));
  rec.rewards = d_rewards; rec.dones = d_dones;
  return launch_env<MODE_ROLLOUT>(w, nullptr, n_steps, 0, 0, 0, 0, 0, first_macro_index, auto_reset, &rec);
}
int rv_rollout_record(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset,
                      float* d_rewards, uint8_t* d_dones, const rv_obs_buffers* step_obs) {
  WCHK(w);
  if (n_steps <= 0) return fail(RV_ERR_VALUE, "rv_rollout_record: n_steps must be positive");
  RolloutRec rec; memset(&rec, 0, sizeof(rec));
  rec.rewards = d_rewards; rec.dones = d_dones;
  float* d_pc = nullptr;
  if (step_obs) {
    rec.obs = *step_obs; rec.has_obs = 1; d_pc = step_obs->d_point_cloud;
    rec.obs.d_point_cloud = nullptr;
  }
  const size_t rows = (size_t)n_steps * (size_t)w->n;
  if (d_pc) {
    if (w->cfg.num_points <= 0 || w->cfg.num_points > RV_PC_MAXPIX) return fail(RV_ERR_VALUE, "rv_rollout_record: num_points outside [1, RV_PC_MAXPIX]");
    int rc = ensure_snaps(w, rows); if (rc != RV_OK) return rc;
    rec.snaps = w->d_snaps;
  }
  PcTail tail; const bool use_tail = d_pc && pc_tail_wanted(w, n_steps);
  if (use_tail) { int rc = pc_tail_setup(w, rows, d_pc, &tail); if (rc != RV_OK) return rc; }
  w->pc_rows = d_pc ? rows : 0; w->pc_flags = use_tail;
  int rc = launch_env<MODE_ROLLOUT>(w, nullptr, n_steps, 0, 0, 0, 0, 0, first_macro_index, auto_reset, &rec, nullptr, nullptr, 0, use_tail ? &tail : nullptr);
  if (rc != RV_OK) return rc;
  // the segmented point clouds of the n_steps x N observations: those the kernel's tail has not rendered, together
  if (d_pc) return launch_point_cloud(w, rows, d_pc, use_tail ? &tail : nullptr);
  return RV_OK;
}
int rv_rollout_record_full(rv_world* w, int32_t n_steps, int32_t first_macro_index, int32_t auto_reset,
                           float* d_rewards, uint8_t* d_dones, const rv_obs_buffers* step_obs, const rv_rollout_extra* extra) {
  WCHK(w);
  if (n_steps <= 0) return fail(RV_ERR_VALUE, "rv_rollout_record_full: n_steps must be positive");
  RolloutRec rec; memset(&rec, 0, sizeof(rec));
  rec.rewards = d_rewards; rec.dones = d_dones;
  float *d_pc = nullptr, *d_rpc = nullptr;
  if (step_obs) { rec.obs = *step_obs; rec.has_obs = 1; d_pc = step_obs->d_point_cloud; rec.obs.d_point_cloud = nullptr; }
  if (extra) {
    rec.actions = extra->d_actions; rec.resets = extra->d_reset;
    rec.robs = extra->reset_obs; rec.has_robs = 1; d_rpc = extra->reset_obs.d_point_cloud; rec.robs.d_point_cloud = nullptr;
  }
  const size_t rows = (size_t)n_steps * (size_t)w->n;
  if (d_pc || d_rpc) {
    if (w->cfg.num_points <= 0 || w->cfg.num_points > RV_PC_MAXPIX) return fail(RV_ERR_VALUE, "rv_rollout_record_full: num_points outside [1, RV_PC_MAXPIX]");
    int rc = ensure_snaps(w, 2 * rows); if (rc != RV_OK) return rc;
    if (d_pc) rec.snaps = w->d_snaps;
    if (d_rpc) {
      rec.rsnaps = w->d_snaps + rows;
      // rows without a reset keep shape = -1 for every body (all bits set): empty clouds
      HIPCHK(hipMemsetAsync(rec.rsnaps, 0xFF, sizeof(ObsSnap) * rows, w->stream));
    }
  }
  if (extra && extra->d_reset) HIPCHK(hipMemsetAsync(extra->d_reset, 0, rows, w->stream));
  PcTail tail; const bool use_tail = d_pc && pc_tail_wanted(w, n_steps);
  if (use_tail) { int rc = pc_tail_setup(w, rows, d_pc, &tail); if (rc != RV_OK) return rc; }
  w->pc_rows = d_pc ? rows : 0; w->pc_flags = use_tail;
  int rc = launch_env<MODE_ROLLOUT>(w, nullptr, n_steps, 0, 0, 0, 0, 0, first_macro_index, auto_reset, &rec, nullptr, nullptr, 0, use_tail ? &tail : nullptr);
  if (rc != RV_OK) return rc;
  if (d_pc) { rc = launch_point_cloud(w, rows, d_pc, use_tail ? &tail : nullptr); if (rc != RV_OK) return rc; }
  if (d_rpc) {      // (the clouds after the resets: all of them here, as ever)
    hipLaunchKernelGGL(k_point_cloud, dim3((unsigned)(rows * RV_MAXB)), dim3(64), 0, w->stream,
                       w->d_snaps + rows, (int)rows, w->n, d_rpc, w->d_cfg, w->d_scene);
    HIPCHK(hipGetLastError());
  }
  return RV_OK;
}
int rv_last_tail_renders(rv_world* w, int32_t* by_tail, int32_t* by_residual) {
  WCHK(w);
  if (!by_tail || !by_residual) return fail(RV_ERR_VALUE, "rv_last_tail_renders: null argument");
  int32_t c[2] = {0, (int32_t)w->pc_rows};      // (no tail in that launch: every row was rendered after the kernel)
  if (w->pc_flags) {
    HIPCHK(hipMemcpyAsync(c, w->d_pc_tail, sizeof(c), hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
  }
  *by_tail = c[0]; *by_residual = c[1];
  return RV_OK;
}
int rv_rollout_async(rv_world* w, int32_t total_env_steps, int32_t first_macro_index, int32_t* d_steps_taken) {
  WCHK(w);
  if (total_env_steps <= 0) return fail(RV_ERR_VALUE, "rv_rollout_async: total_env_steps must be positive");
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(1), 0, w->stream, w->d_budget, (int)total_env_steps);
  HIPCHK(hipGetLastError());
  return launch_env<MODE_ROLLOUT>(w, nullptr, 0, 0, 0, 0, 0, 0, first_macro_index, 1, nullptr, w->d_budget, d_steps_taken, (long long)total_env_steps);
}
int rv_step_begin(rv_world* w, const float* d_actions, const uint8_t* d_mask) {
  WCHK(w);
  if (!d_actions) return fail(RV_ERR_VALUE, "rv_step_begin: null buffer");
  const int G = w->cfg.num_goal_steps > 0 ? w->cfg.num_goal_steps : 1;
  hipLaunchKernelGGL(k_step_begin, grid1(w->n), dim3(TPB), 0, w->stream, w->d_envs, w->n, d_actions, d_mask, G);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_set_auto_reset(rv_world* w, int32_t on) { WCHK(w); w->auto_reset = on != 0; return RV_OK; }
int rv_step_poll(rv_world* w, int32_t max_substeps, int32_t max_usec, uint8_t* d_finished,
                 const rv_obs_buffers* obs, float* d_reward, uint8_t* d_done) {
  WCHK(w);
  if (!d_finished) return fail(RV_ERR_VALUE, "rv_step_poll: null buffer");
  if (max_substeps < 0 || max_usec < 0) return fail(RV_ERR_VALUE, "rv_step_poll: negative budget");
  EnvKernelArgs a;
  memset(&a, 0, sizeof(a));
  a.cfg = w->d_cfg; a.scene = w->d_scene; a.envs = w->d_envs; a.n_envs = w->n;
  a.n_substeps = max_substeps; a.finished = d_finished; a.auto_reset = w->auto_reset;
  poison_range(a);
  a.rec.rewards = d_reward; a.rec.dones = d_done;
  float* d_pc = nullptr;
  if (obs) {
    a.rec.obs = *obs; a.rec.has_obs = 1; d_pc = obs->d_point_cloud; a.rec.obs.d_point_cloud = nullptr;
    if (d_pc) {
      if (w->cfg.num_points <= 0 || w->cfg.num_points > RV_PC_MAXPIX) return fail(RV_ERR_VALUE, "rv_step_poll: num_points outside [1, RV_PC_MAXPIX]");
      int rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
      a.rec.snaps = w->d_snaps;
      HIPCHK(hipMemsetAsync(w->d_snaps, 0xFF, sizeof(ObsSnap) * (size_t)w->n, w->stream));   // shape = -1: no cloud for envs that do not finish
    }
  }
  if (max_usec > 0) {
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, w->device));   // s_memtime ticks at the shader clock on gfx950
    a.budget_clk = (unsigned long long)max_usec * (unsigned long long)(khz > 0 ? khz : 2400000) / 1000ull;
  }
  HIPCHK(hipMemsetAsync(w->d_stats, 0, sizeof(rv_macro_stats), w->stream));
  HIPCHK(hipEventRecord(w->ev0, w->stream));
  launch_k_env(w, MODE_PARTIAL, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(w->ev1, w->stream));
  w->timed = true;
  hipLaunchKernelGGL(k_stats, grid1(w->n), dim3(TPB), 0, w->stream, w->d_envs, w->n, w->d_stats, w->cfg.success_thresh);
  HIPCHK(hipGetLastError());
  if (d_pc) return launch_point_cloud(w, (size_t)w->n, d_pc);
  return RV_OK;
}
int rv_step_sub(rv_world* w, int32_t n) {
  WCHK(w);
  if (n < 0) return fail(RV_ERR_VALUE, "rv_step_sub: negative substep count");
  return launch_env<MODE_SUB>(w, nullptr, n, 0, 0, 0, 0, 0);
}
int rv_wait_until_stable(rv_world* w, float lin, float ang, int32_t ca, int32_t ms, int32_t mx) {
  WCHK(w);
  if (mx <= 0) return fail(RV_ERR_VALUE, "rv_wait_until_stable: max_steps must be positive");
  return launch_env<MODE_WAIT>(w, nullptr, 0, lin, ang, ca, ms, mx);
}

#define SIMPLE_LAUNCH(kern, ...) do { hipLaunchKernelGGL(kern, grid1(w->n), dim3(TPB), 0, w->stream, __VA_ARGS__); HIPCHK(hipGetLastError()); } while (0)
#define NEED(p, name) do { if (!(p)) return fail(RV_ERR_VALUE, name ": null buffer"); } while (0)

int rv_set_actions(rv_world* w, const float* d) {
  WCHK(w); NEED(d, "rv_set_actions");
  int G = w->cfg.num_goal_steps > 0 ? w->cfg.num_goal_steps : 1;
  SIMPLE_LAUNCH(k_set_actions, w->d_envs, w->n, d, G); return RV_OK;
}
int rv_policy_random(rv_world* w, int32_t macro_index, float* d) {
  WCHK(w); NEED(d, "rv_policy_random");
  SIMPLE_LAUNCH(k_policy_random, w->n, w->d_cfg, macro_index, d); return RV_OK;
}
int rv_policy_heuristic(rv_world* w, int32_t max_attempts, float* d) {
  WCHK(w); NEED(d, "rv_policy_heuristic");
  if (max_attempts <= 0) return fail(RV_ERR_VALUE, "rv_policy_heuristic: max_attempts must be positive");
  hipLaunchKernelGGL(k_policy_heuristic, dim3((unsigned)w->n), dim3(64), 0, w->stream, w->d_envs, w->n, w->d_cfg, max_attempts, d);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_get_body_state(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_body_state"); SIMPLE_LAUNCH(k_get_body_state, w->d_envs, w->n, d); return RV_OK; }
int rv_set_body_state(rv_world* w, const float* d) { WCHK(w); NEED(d, "rv_set_body_state"); SIMPLE_LAUNCH(k_set_body_state, w->d_envs, w->n, d); return RV_OK; }
int rv_get_body_params(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_body_params"); SIMPLE_LAUNCH(k_get_body_params, w->d_envs, w->n, d); return RV_OK; }
int rv_set_body_params(rv_world* w, const float* d) { WCHK(w); NEED(d, "rv_set_body_params"); SIMPLE_LAUNCH(k_set_body_params, w->d_envs, w->n, d, w->d_cfg, w->d_scene); return RV_OK; }
int rv_get_joint_state(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_joint_state"); SIMPLE_LAUNCH(k_get_joint_state, w->d_envs, w->n, d); return RV_OK; }
int rv_set_joint_state(rv_world* w, const float* d) { WCHK(w); NEED(d, "rv_set_joint_state"); SIMPLE_LAUNCH(k_set_joint_state, w->d_envs, w->n, d, w->d_cfg, w->d_scene); return RV_OK; }
int rv_get_link_poses(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_link_poses"); SIMPLE_LAUNCH(k_get_link_poses, w->d_envs, w->n, d); return RV_OK; }
#ifdef RV_PROFILE
// profiling build only (tools/prof_rollout.py): per-env shader-clock time per substep part
int rv_debug_profile(rv_world* w, unsigned long long* d) { WCHK(w); NEED(d, "rv_debug_profile"); SIMPLE_LAUNCH(k_debug_profile, w->d_envs, w->n, d); return RV_OK; }
#endif
int rv_get_env_counters(rv_world* w, int32_t* d) { WCHK(w); NEED(d, "rv_get_env_counters"); SIMPLE_LAUNCH(k_get_env_counters, w->d_envs, w->n, d); return RV_OK; }
int rv_set_joint_targets(rv_world* w, const float* d, float timeout, float threshold) { WCHK(w); NEED(d, "rv_set_joint_targets"); SIMPLE_LAUNCH(k_set_joint_targets, w->d_envs, w->n, d, w->d_cfg, w->d_scene, timeout, threshold); return RV_OK; }
int rv_set_link_target(rv_world* w, const float* d, float timeout, float threshold) { WCHK(w); NEED(d, "rv_set_link_target"); SIMPLE_LAUNCH(k_set_link_target, w->d_envs, w->n, d, w->d_cfg, w->d_scene, timeout, threshold); return RV_OK; }
int rv_set_link_path(rv_world* w, const float* d, int32_t n_poses, float timeout, float threshold) {
  WCHK(w); NEED(d, "rv_set_link_path");
  if (n_poses < 1 || n_poses > RV_MAXQ) return fail(RV_ERR_VALUE, "rv_set_link_path: 1 <= n_poses <= RV_MAXQ");
  SIMPLE_LAUNCH(k_set_link_path, w->d_envs, w->n, d, n_poses, w->d_cfg, w->d_scene, timeout, threshold); return RV_OK;
}
int rv_set_max_joint_velocities(rv_world* w, const float* d) {
  WCHK(w); NEED(d, "rv_set_max_joint_velocities");
  SIMPLE_LAUNCH(k_set_max_joint_velocities, w->d_envs, w->n, d); return RV_OK;
}
int rv_get_camera(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_camera"); SIMPLE_LAUNCH(k_get_camera, w->d_envs, w->n, d); return RV_OK; }
int rv_get_robot_ready(rv_world* w, uint8_t* d) { WCHK(w); NEED(d, "rv_get_robot_ready"); SIMPLE_LAUNCH(k_robot_ready, w->d_envs, w->n, d, w->d_cfg); return RV_OK; }
int rv_set_motor_targets(rv_world* w, const float* d_q, const uint8_t* d_mask) {
  WCHK(w); NEED(d_q, "rv_set_motor_targets");
  SIMPLE_LAUNCH(k_set_motor_targets, w->d_envs, w->n, d_q, d_mask, w->d_cfg); return RV_OK;
}
int rv_set_gravity(rv_world* w, const float* g) {
  WCHK(w); NEED(g, "rv_set_gravity");
  w->cfg.gravity_xy[0] = g[0]; w->cfg.gravity_xy[1] = g[1]; w->cfg.gravity_z = g[2];
  HIPCHK(hipMemcpyAsync(w->d_cfg, &w->cfg, sizeof(rv_config), hipMemcpyHostToDevice, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  return RV_OK;
}
int rv_set_friction(rv_world* w, float mu_finger, float mu_table) {
  WCHK(w);
  SIMPLE_LAUNCH(k_set_friction, w->d_envs, w->n, mu_finger, mu_table);
  return RV_OK;
}
int rv_set_constraint_ex(rv_world* w, int32_t body, int32_t child, int32_t joint_type, const float* frame7, const float* child_frame7, float max_force) {
  WCHK(w);
  if (body < 0 || body >= RV_MAXB) return fail(RV_ERR_VALUE, "rv_set_constraint: not a movable body slot");
  if (child < -1 || child >= RV_MAXB + RV_NFRAME || child == body) return fail(RV_ERR_VALUE, "rv_set_constraint: the child is the world (-1), another movable body slot or RV_CHILD_LINK(frame)");
  if (child >= RV_MAXB && joint_type != RV_JOINT_FIXED && joint_type != RV_JOINT_POINT2POINT) return fail(RV_ERR_NOTIMPL, "rv_set_constraint: a link of the arm as the other party: fixed and point2point joints");
  if (joint_type != RV_JOINT_FIXED && joint_type != RV_JOINT_POINT2POINT && joint_type != RV_JOINT_PRISMATIC && joint_type != RV_JOINT_REVOLUTE) return fail(RV_ERR_NOTIMPL, "rv_set_constraint: joint types built: fixed, point2point, prismatic, revolute");
  if (max_force >= 0.0f && !child_frame7) return fail(RV_ERR_VALUE, "rv_set_constraint: null target");
  ConArgs a; memset(&a, 0, sizeof(a));
  a.body = body; a.child = child; a.type = joint_type == RV_JOINT_POINT2POINT ? 2 : (joint_type == RV_JOINT_PRISMATIC ? 3 : (joint_type == RV_JOINT_REVOLUTE ? 4 : 1)); a.fmax = max_force; a.lq[3] = 1.0f; a.tq[3] = 1.0f;
  if (max_force >= 0.0f) {
    if (frame7) { for (int k = 0; k < 3; ++k) a.lp[k] = frame7[k]; for (int k = 0; k < 4; ++k) a.lq[k] = frame7[3 + k]; }
    for (int k = 0; k < 3; ++k) a.tp[k] = child_frame7[k];
    for (int k = 0; k < 4; ++k) a.tq[k] = child_frame7[3 + k];
  }
  SIMPLE_LAUNCH(k_set_constraint, w->d_envs, w->n, a);
  return RV_OK;
}
int rv_set_constraint(rv_world* w, int32_t body, const float* frame7, const float* target7, float max_force) {
  return rv_set_constraint_ex(w, body, -1, RV_JOINT_FIXED, frame7, target7, max_force);
}
int rv_grip(rv_world* w, float value) { WCHK(w); SIMPLE_LAUNCH(k_grip, w->d_envs, w->n, value, w->d_cfg, w->d_scene); return RV_OK; }
int rv_reset_targets(rv_world* w) { WCHK(w); SIMPLE_LAUNCH(k_reset_targets, w->d_envs, w->n); return RV_OK; }
int rv_get_state_ptrs(rv_world* w, rv_state_view* v) {
  WCHK(w); NEED(v, "rv_get_state_ptrs");
  v->d_envs = w->d_envs; v->env_stride_bytes = (int64_t)sizeof(DevEnv);
  v->off_body = (int64_t)offsetof(DevEnv, body); v->off_active = (int64_t)offsetof(DevEnv, active);
  v->off_joint_q = (int64_t)offsetof(DevEnv, q); v->off_joint_qd = (int64_t)offsetof(DevEnv, qd);
  v->off_link_pos = (int64_t)offsetof(DevEnv, fpos); v->off_link_quat = (int64_t)offsetof(DevEnv, fquat);
  v->off_obs_pos = (int64_t)offsetof(DevEnv, obs_pos); v->off_table_z = (int64_t)offsetof(DevEnv, table_z);
  return RV_OK;
}
#ifndef RV_SOURCE_HASH
#define RV_SOURCE_HASH "unknown"
#endif
const char* rv_source_hash(void) { return RV_SOURCE_HASH; }
int rv_compute_ik(rv_world* w, const float* d_pose, float* d_q) {
  WCHK(w); NEED(d_pose, "rv_compute_ik"); NEED(d_q, "rv_compute_ik");
  SIMPLE_LAUNCH(k_compute_ik, w->d_envs, w->n, d_pose, d_q, w->d_cfg, w->d_scene); return RV_OK;
}
int rv_query_contacts(rv_world* w, uint8_t* d) { WCHK(w); NEED(d, "rv_query_contacts"); SIMPLE_LAUNCH(k_query_contacts, w->d_envs, w->n, d); return RV_OK; }
int rv_get_contact_points(rv_world* w, const rv_contact_query* q, int capacity, int32_t* d_ids, float* d_data, int32_t* d_count) {
  WCHK(w); NEED(q, "rv_get_contact_points"); NEED(d_ids, "rv_get_contact_points"); NEED(d_data, "rv_get_contact_points"); NEED(d_count, "rv_get_contact_points");
  if (capacity < 1 || capacity > RV_CP_MAX) return fail(RV_ERR_VALUE, "rv_get_contact_points: capacity outside [1, RV_CP_MAX]");
  const int body[2] = {q->body_a, q->body_b}, link[2] = {q->link_a, q->link_b};
  for (int s = 0; s < 2; ++s) {
    if (body[s] < -1 || body[s] > RV_CP_ARM) return fail(RV_ERR_VALUE, "rv_get_contact_points: unknown body code " + std::to_string(body[s]));
    if (link[s] < -1 || link[s] >= RV_NFRAME) return fail(RV_ERR_VALUE, "rv_get_contact_points: link outside [-1, RV_NFRAME)");
    if (link[s] >= 0 && body[s] != RV_CP_ARM) return fail(RV_ERR_VALUE, "rv_get_contact_points: a link index is only meaningful for the arm (RV_CP_ARM)");
  }
  CpArgs a; a.q = *q; a.capacity = capacity; a.ids = d_ids; a.data = d_data; a.count = d_count;
  hipLaunchKernelGGL(k_contact_points, dim3((unsigned)((w->n + RV_CP_WAVES - 1) / RV_CP_WAVES)), dim3(64 * RV_CP_WAVES), 0, w->stream,
                     w->d_envs, w->n, w->d_cfg, w->d_scene, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_get_manifold_counts(rv_world* w, int32_t* d) { WCHK(w); NEED(d, "rv_get_manifold_counts"); SIMPLE_LAUNCH(k_manifold_counts, w->d_envs, w->n, d); return RV_OK; }
int rv_observe(rv_world* w, const rv_obs_buffers* obs) {
  WCHK(w); NEED(obs, "rv_observe");
  SIMPLE_LAUNCH(k_observe, w->d_envs, w->n, *obs, w->d_cfg);
  if (obs->d_point_cloud) {
    if (w->cfg.num_points <= 0 || w->cfg.num_points > RV_PC_MAXPIX) return fail(RV_ERR_VALUE, "rv_observe: num_points outside [1, RV_PC_MAXPIX]");
    int rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
    SIMPLE_LAUNCH(k_obs_snap, w->d_envs, w->n, w->d_snaps, w->d_scene);
    rc = launch_point_cloud(w, w->n, obs->d_point_cloud); if (rc != RV_OK) return rc;
  }
  return RV_OK;
}
int rv_render_rgb(rv_world* w, uint8_t* d_rgb) {
  WCHK(w); NEED(d_rgb, "rv_render_rgb");
  int rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
  SIMPLE_LAUNCH(k_obs_snap, w->d_envs, w->n, w->d_snaps, w->d_scene);
  const size_t total = (size_t)w->n * (size_t)w->cfg.cam_height * (size_t)w->cfg.cam_width;
  hipLaunchKernelGGL(k_render_rgb, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, w->stream, w->d_snaps, w->n, d_rgb, w->d_cfg, w->d_scene);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_render(rv_world* w, float* d_depth, uint8_t* d_segmask) {
  WCHK(w);
  if (!d_depth && !d_segmask) return fail(RV_ERR_VALUE, "rv_render: no output buffer");
  int rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
  SIMPLE_LAUNCH(k_obs_snap, w->d_envs, w->n, w->d_snaps, w->d_scene);
  const size_t total = (size_t)w->n * (size_t)w->cfg.cam_height * (size_t)w->cfg.cam_width;
  hipLaunchKernelGGL(k_render, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, w->stream, w->d_snaps, w->n, d_depth, d_segmask, w->d_cfg, w->d_scene);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_render_view(rv_world* w, const rv_view_params* p, const int32_t* h_env_index, const float* h_cameras,
                   uint8_t* d_rgb, float* d_depth, uint8_t* d_segmask) {
  WCHK(w);
  if (!p || !h_env_index || !h_cameras) return fail(RV_ERR_VALUE, "rv_render_view: null params, env index or cameras");
  if (!d_rgb && !d_depth && !d_segmask) return fail(RV_ERR_VALUE, "rv_render_view: no output buffer");
  if (p->n_views < 1 || p->n_views > RV_VIEW_MAX_VIEWS) return fail(RV_ERR_VALUE, "rv_render_view: n_views outside [1, RV_VIEW_MAX_VIEWS]");
  if (p->height < 1 || p->height > RV_VIEW_MAX_SIDE || p->width < 1 || p->width > RV_VIEW_MAX_SIDE)
    return fail(RV_ERR_VALUE, "rv_render_view: height or width outside [1, RV_VIEW_MAX_SIDE]");
  if (p->supersample < 1 || p->supersample > RV_VIEW_MAX_SUPERSAMPLE) return fail(RV_ERR_VALUE, "rv_render_view: supersample outside [1, RV_VIEW_MAX_SUPERSAMPLE]");
  if (p->supersample > 1 && (d_depth || d_segmask)) return fail(RV_ERR_VALUE, "rv_render_view: supersampling is for rgb only (no depth or segmask with supersample > 1)");
  if (d_depth && !aligned_to(d_depth, 4)) return fail(RV_ERR_VALUE, "rv_render_view: d_depth must be 4-byte aligned");
  const size_t V = (size_t)p->n_views;
  for (size_t k = 0; k < V; ++k) {
    if (h_env_index[k] < 0 || h_env_index[k] >= w->n) return fail(RV_ERR_VALUE, "rv_render_view: env index " + std::to_string(h_env_index[k]) + " of view " + std::to_string(k) + " outside [0, N)");
    const float* r = h_cameras + k * 17;
    for (int j = 0; j < 17; ++j)      // (x - x is 0 for a finite x and NaN otherwise)
      if (!(r[j] - r[j] == 0.0f)) return fail(RV_ERR_VALUE, "rv_render_view: camera row " + std::to_string(k) + " has a non-finite entry");
    if (r[0] == 0.0f || r[1] == 0.0f) return fail(RV_ERR_VALUE, "rv_render_view: camera row " + std::to_string(k) + " has fx == 0 or fy == 0");
  }
  // the indices and the rows (scaled to the supersampled image, in float32) as one block: [V] int32, [V][17] float
  const size_t bytes = V * sizeof(int32_t) + V * 17 * sizeof(float);
  if (w->view_cap < bytes) {
    HIPCHK(hipStreamSynchronize(w->stream));
    if (w->d_view) { HIPCHK(hipFree(w->d_view)); w->d_view = nullptr; }
    if (w->h_view) { HIPCHK(hipHostFree(w->h_view)); w->h_view = nullptr; }
    w->view_cap = 0; w->view_bytes = 0;
    HIPCHK(hipMalloc(&w->d_view, bytes));
    HIPCHK(hipHostMalloc(&w->h_view, bytes, hipHostMallocDefault));
    w->view_cap = bytes;
  }
  std::vector<uint8_t> block(bytes);
  {
    int32_t* idx = reinterpret_cast<int32_t*>(block.data());
    float* rows = reinterpret_cast<float*>(block.data() + V * sizeof(int32_t));
    const float s = (float)p->supersample, off = 0.5f * (float)(p->supersample - 1);
    for (size_t k = 0; k < V; ++k) {
      idx[k] = h_env_index[k];
      const float* r = h_cameras + k * 17; float* o = rows + k * 17;
      for (int j = 0; j < 17; ++j) o[j] = r[j];
      if (p->supersample > 1) { o[0] = s * r[0]; o[1] = s * r[1]; o[4] = s * r[4]; o[2] = s * r[2] + off; o[3] = s * r[3] + off; }
    }
  }
  if (w->view_bytes != bytes || memcmp(w->h_view, block.data(), bytes) != 0) {
    if (w->view_bytes) HIPCHK(hipEventSynchronize(w->ev_view));      // the previous upload still reads the pinned copy
    w->view_bytes = 0;
    memcpy(w->h_view, block.data(), bytes);
    HIPCHK(hipMemcpyAsync(w->d_view, w->h_view, bytes, hipMemcpyHostToDevice, w->stream));
    HIPCHK(hipEventRecord(w->ev_view, w->stream));
    w->view_bytes = bytes;
  }
  int rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
  SIMPLE_LAUNCH(k_obs_snap, w->d_envs, w->n, w->d_snaps, w->d_scene);
  ViewArgs a;
  a.snaps = w->d_snaps; a.env_index = reinterpret_cast<const int32_t*>(w->d_view);
  a.cameras = reinterpret_cast<const float*>(w->d_view + V * sizeof(int32_t));
  a.height = p->height; a.width = p->width; a.ss = p->supersample;
  a.rgb = d_rgb; a.depth = d_depth; a.seg = d_segmask;
  const size_t per_view = (size_t)p->height * (size_t)p->width;
  const size_t per_group = (size_t)RV_VIEW_TPB * RV_VIEW_PPT;
  hipLaunchKernelGGL(k_render_view, dim3((unsigned)((per_view + per_group - 1) / per_group), (unsigned)V), dim3(RV_VIEW_TPB), 0, w->stream,
                     a, w->d_cfg, w->d_scene);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
// the checks of the sampler's parameters against an H x W image, and the geometry they give (rv_grasp_refine shares them)
static int antipodal_geometry(const rv_antipodal_params& p, int H, int W, const std::string& fn, ApArgs* out) {
  if (p.downsample_rate < 1 || p.downsample_rate > 8) return fail(RV_ERR_VALUE, fn + ": DOWNSAMPLE_RATE must be an integer in 1..8");
  if (p.depth_samples_per_grasp != 1) return fail(RV_ERR_VALUE, fn + ": DEPTH_SAMPLES_PER_GRASP must be 1 (one depth per grasp)");
  if (p.max_rejection_samples < 1) return fail(RV_ERR_VALUE, fn + ": MAX_REJECTION_SAMPLES must be positive");
  if (p.gauss_radius < 0 || p.gauss_radius > RV_AP_MAX_RADIUS) return fail(RV_ERR_VALUE, fn + ": Gaussian radius int(4 sigma + 0.5) outside [0, RV_AP_MAX_RADIUS]");
  const float wh = p.depth_sample_window_height, ww = p.depth_sample_window_width;
  if (!(wh >= 1.0f && ww >= 1.0f && p.min_dist_from_boundary > (wh > ww ? wh : ww)))
    return fail(RV_ERR_VALUE, fn + ": need MIN_DIST_FROM_BOUNDARY > max(DEPTH_SAMPLE_WINDOW_HEIGHT, DEPTH_SAMPLE_WINDOW_WIDTH) >= 1");
  if (!(p.cone_cos >= 0.0f && p.cone_cos <= 1.0f)) return fail(RV_ERR_VALUE, fn + ": cone_cos = cos(arctan(FRICTION_COEF)) outside [0, 1]");
  int r0 = 0, c0 = 0, r1 = H, c1 = W;
  if (p.use_crop) { r0 = p.crop[0]; c0 = p.crop[1]; r1 = p.crop[2]; c1 = p.crop[3]; }
  if (!(0 <= r0 && r0 < r1 && r1 <= H && 0 <= c0 && c0 < c1 && c1 <= W)) return fail(RV_ERR_VALUE, fn + ": CROP must be 0 <= r0 < r1 <= H, 0 <= c0 < c1 <= W");
  ApArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.H = H; a.W = W; a.r0 = r0; a.c0 = c0; a.Hc = r1 - r0; a.Wc = c1 - c0;
  a.Hd = a.Hc / p.downsample_rate; a.Wd = a.Wc / p.downsample_rate;
  if (a.Hd < 2 || a.Wd < 2) return fail(RV_ERR_VALUE, fn + ": the downsampled crop must be at least 2 x 2");
  *out = a;
  return RV_OK;
}
// the checks and the launch arguments the two antipodal entry points share (`fn`: the entry point the message names)
static int antipodal_args(rv_world* w, const float* d_depth, const rv_antipodal_params* h_params, int32_t macro_index,
                          const std::string& fn, ApArgs* out) {
  if (w->cfg.env_type != RV_ENV_GRASP) return fail(RV_ERR_VALUE, fn + ": a Grasp4DofEnv world only");
  const int H = w->cfg.cam_height, W = w->cfg.cam_width;
  ApArgs a;
  int rc = antipodal_geometry(*h_params, H, W, fn, &a); if (rc != RV_OK) return rc;
  a.macro_index = macro_index;
  if (!d_depth) {
    int rc = ensure_floats(w, &w->d_ap_depth, &w->ap_depth_cap, (size_t)w->n * H * W); if (rc != RV_OK) return rc;
    rc = rv_render(w, w->d_ap_depth, nullptr); if (rc != RV_OK) return rc;
    d_depth = w->d_ap_depth;
  }
  rc = ensure_floats(w, &w->d_ap_scratch, &w->ap_scratch_cap, (size_t)w->n * 2 * a.Hc * a.Wc); if (rc != RV_OK) return rc;
  a.depth = d_depth; a.scratch = w->d_ap_scratch;
  *out = a;
  return RV_OK;
}
int rv_policy_antipodal(rv_world* w, const float* d_depth, const rv_antipodal_params* h_params, int32_t macro_index,
                        float* d_image_grasps, float* d_actions4, int32_t* d_status) {
  WCHK(w); NEED(h_params, "rv_policy_antipodal"); NEED(d_image_grasps, "rv_policy_antipodal"); NEED(d_status, "rv_policy_antipodal");
  ApArgs a;
  int rc = antipodal_args(w, d_depth, h_params, macro_index, "rv_policy_antipodal", &a); if (rc != RV_OK) return rc;
  a.grasps = d_image_grasps; a.actions4 = d_actions4; a.status = d_status;
  hipLaunchKernelGGL(k_policy_antipodal, dim3((unsigned)w->n), dim3(RV_AP_TPB), 0, w->stream, w->d_envs, w->n, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_policy_antipodal_multi(rv_world* w, const float* d_depth, const rv_antipodal_params* h_params, int32_t macro_index,
                              int32_t num_samples, float* d_image_grasps, float* d_actions4, int32_t* d_count, int32_t* d_status) {
  WCHK(w); NEED(h_params, "rv_policy_antipodal_multi"); NEED(d_image_grasps, "rv_policy_antipodal_multi");
  NEED(d_count, "rv_policy_antipodal_multi"); NEED(d_status, "rv_policy_antipodal_multi");
  if (num_samples < 1 || num_samples > RV_AP_MAX_SAMPLES) return fail(RV_ERR_VALUE, "rv_policy_antipodal_multi: num_samples outside [1, RV_AP_MAX_SAMPLES]");
  ApArgs a;
  int rc = antipodal_args(w, d_depth, h_params, macro_index, "rv_policy_antipodal_multi", &a); if (rc != RV_OK) return rc;
  a.grasps = d_image_grasps; a.actions4 = d_actions4; a.status = d_status; a.num_samples = num_samples; a.count = d_count;
  hipLaunchKernelGGL(k_policy_antipodal_multi, dim3((unsigned)w->n), dim3(RV_AP_TPB), 0, w->stream, w->d_envs, w->n, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_plan_reward(rv_world* w, const rv_plan_params* h_params, const float* d_state, const float* d_next_state,
                   int64_t m, float* d_reward, uint8_t* d_termination) {
  WCHK(w);
  int rc = plan_check(w, h_params, "rv_plan_reward"); if (rc != RV_OK) return rc;
  if (m < 0) return fail(RV_ERR_VALUE, "rv_plan_reward: m must not be negative");
  if (m == 0) return RV_OK;
  NEED(d_state, "rv_plan_reward"); NEED(d_next_state, "rv_plan_reward"); NEED(d_reward, "rv_plan_reward"); NEED(d_termination, "rv_plan_reward");
  if (!aligned_to(d_state, 8) || !aligned_to(d_next_state, 8)) return fail(RV_ERR_VALUE, "rv_plan_reward: the state buffers must be 8-byte aligned");
  if ((m + 255) / 256 > 0x7fffffffLL) return fail(RV_ERR_VALUE, "rv_plan_reward: m too large for one launch");
  const bool v4 = aligned_to(d_state, 16) && aligned_to(d_next_state, 16);
  const rv_plan_params p = *h_params;
  PLAN_DISPATCH(p.n_bodies, v4, launch_plan_reward, w, p, d_state, d_next_state, (long long)m, d_reward, d_termination);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_plan_score(rv_world* w, const rv_plan_params* h_params, const float* d_state0, const float* d_plans,
                  int32_t s, int32_t h, float* d_returns, int32_t* d_lengths, int32_t* d_best) {
  WCHK(w);
  int rc = plan_check(w, h_params, "rv_plan_score"); if (rc != RV_OK) return rc;
  if (s < 1 || h < 1) return fail(RV_ERR_VALUE, "rv_plan_score: s and h must be positive");
  NEED(d_plans, "rv_plan_score");
  if (!aligned_to(d_plans, 8) || !aligned_to(d_state0, 8)) return fail(RV_ERR_VALUE, "rv_plan_score: the plan and state buffers must be 8-byte aligned");
  PlanArgs a;
  a.p = *h_params; a.state0 = d_state0; a.plans = d_plans; a.S = s; a.H = h;
  a.returns = d_returns; a.lengths = d_lengths; a.best = d_best;
  // one workgroup per env; as many waves as the env has plans for, 16 at the most (a lane then walks several plans)
  const int tpb = s <= 64 ? 64 : (s <= 256 ? 256 : RV_PLAN_MAX_TPB);
  const bool v4 = aligned_to(d_plans, 16);
  PLAN_DISPATCH(a.p.n_bodies, v4, launch_plan_score, w, a, tpb);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
// the checks rv_cem_sample and rv_cem_refit share; *d = h * G * 4
static int cem_check(const rv_world* w, const rv_cem_params* p, int32_t s, int32_t h, const std::string& me, int* d) {
  if (!p) return fail(RV_ERR_VALUE, me + ": null params");
  if (w->cfg.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, me + ": a PushEnv world only");
  if (s < 1 || s > RV_CEM_MAX_SAMPLES) return fail(RV_ERR_VALUE, me + ": s outside [1, RV_CEM_MAX_SAMPLES]");
  const int A = 4 * (w->cfg.num_goal_steps > 0 ? w->cfg.num_goal_steps : 1);
  if (h < 1 || (long long)h * A > RV_CEM_MAX_DIM) return fail(RV_ERR_VALUE, me + ": h < 1 or h * G * 4 > RV_CEM_MAX_DIM");
  if (p->plan_index < 0 || p->plan_index >= RV_CEM_MAX_PLAN_INDEX) return fail(RV_ERR_VALUE, me + ": plan_index outside [0, 2^24)");
  if (p->iteration < 0 || p->iteration >= RV_CEM_MAX_ITERATION) return fail(RV_ERR_VALUE, me + ": iteration outside [0, 2^15)");
  *d = h * A;
  return RV_OK;
}
int rv_cem_sample(rv_world* w, const rv_cem_params* h_params, const float* d_mean, const float* d_std,
                  int32_t s, int32_t h, float* d_actions) {
  WCHK(w);
  CemArgs a;
  int rc = cem_check(w, h_params, s, h, "rv_cem_sample", &a.D); if (rc != RV_OK) return rc;
  NEED(d_mean, "rv_cem_sample"); NEED(d_std, "rv_cem_sample"); NEED(d_actions, "rv_cem_sample");
  if (!aligned_to(d_mean, 4) || !aligned_to(d_std, 4) || !aligned_to(d_actions, 4)) return fail(RV_ERR_VALUE, "rv_cem_sample: the buffers must be 4-byte aligned");
  const long long total = (long long)w->n * s * (a.D / 4);      // one lane per four floats
  if ((total + 255) / 256 > 0x7fffffffLL) return fail(RV_ERR_VALUE, "rv_cem_sample: too many candidates for one launch");
  a.p = *h_params; a.actions = nullptr; a.returns = nullptr; a.elite = nullptr; a.S = s;
  a.mean = const_cast<float*>(d_mean); a.std = const_cast<float*>(d_std); a.out = d_actions;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (aligned_to(d_actions, 16)) hipLaunchKernelGGL(k_cem_sample<true>, grid, dim3(256), 0, w->stream, w->d_cfg, a, total);
  else hipLaunchKernelGGL(k_cem_sample<false>, grid, dim3(256), 0, w->stream, w->d_cfg, a, total);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_cem_refit(rv_world* w, const rv_cem_params* h_params, const float* d_actions, const float* d_returns,
                 int32_t s, int32_t h, float* d_mean, float* d_std, int32_t* d_elite) {
  WCHK(w);
  CemArgs a;
  int rc = cem_check(w, h_params, s, h, "rv_cem_refit", &a.D); if (rc != RV_OK) return rc;
  if (h_params->n_elites < 1 || h_params->n_elites > s) return fail(RV_ERR_VALUE, "rv_cem_refit: n_elites outside [1, s]");
  if (!(h_params->alpha >= 0.0f && h_params->alpha < 1.0f)) return fail(RV_ERR_VALUE, "rv_cem_refit: alpha outside [0, 1)");
  if (!(h_params->min_std >= 0.0f)) return fail(RV_ERR_VALUE, "rv_cem_refit: min_std negative or NaN");
  NEED(d_actions, "rv_cem_refit"); NEED(d_returns, "rv_cem_refit"); NEED(d_mean, "rv_cem_refit"); NEED(d_std, "rv_cem_refit");
  if (!aligned_to(d_actions, 4) || !aligned_to(d_returns, 4) || !aligned_to(d_mean, 4) || !aligned_to(d_std, 4) || !aligned_to(d_elite, 4))
    return fail(RV_ERR_VALUE, "rv_cem_refit: the buffers must be 4-byte aligned");
  a.p = *h_params; a.actions = d_actions; a.returns = d_returns; a.mean = d_mean; a.std = d_std; a.out = nullptr;
  a.elite = d_elite; a.S = s;
  // one workgroup per env, k_plan_score's shapes
  const int tpb = s <= 64 ? 64 : (s <= 256 ? 256 : RV_CEM_MAX_TPB);
  hipLaunchKernelGGL(k_cem_refit, dim3((unsigned)w->n), dim3((unsigned)tpb), 0, w->stream, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_depth_noise(rv_world* w, const rv_depth_noise_params* h_params, const float* d_depth_in, float* d_depth_out,
                   float* d_gamma, uint8_t* d_applied, float* d_grid) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_depth_noise: null params");
  NEED(d_depth_in, "rv_depth_noise"); NEED(d_depth_out, "rv_depth_noise");
  const rv_depth_noise_params& p = *h_params;
  if (!aligned_to(d_depth_in, 4) || !aligned_to(d_depth_out, 4) || !aligned_to(d_gamma, 4) || !aligned_to(d_grid, 4))
    return fail(RV_ERR_VALUE, "rv_depth_noise: the buffers must be 4-byte aligned");
  if (p.height < 1 || p.width < 1) return fail(RV_ERR_VALUE, "rv_depth_noise: height or width < 1");
  const int R = p.rescale_factor;
  if (R < 1 || R > RV_DN_MAX_RESCALE) return fail(RV_ERR_VALUE, "rv_depth_noise: rescale_factor outside [1, 8]");
  if (p.height % R != 0 || p.width % R != 0) return fail(RV_ERR_VALUE, "rv_depth_noise: rescale_factor must divide height and width");
  if (p.draw_index < 0 || p.draw_index >= RV_DN_MAX_DRAW_INDEX) return fail(RV_ERR_VALUE, "rv_depth_noise: draw_index outside [0, 2^24)");
  if (!(p.gamma_shape == 0.0f || p.gamma_shape >= 1.0f)) return fail(RV_ERR_VALUE, "rv_depth_noise: gamma_shape must be 0 (off) or >= 1");
  if (!(p.prob >= 0.0f && p.prob <= 1.0f)) return fail(RV_ERR_VALUE, "rv_depth_noise: prob outside [0, 1]");
  if (!(p.sigma >= 0.0f)) return fail(RV_ERR_VALUE, "rv_depth_noise: sigma negative or NaN");
  DnArgs a;
  a.p = p; a.in = d_depth_in; a.out = d_depth_out; a.gamma_out = d_gamma; a.applied_out = d_applied;
  a.h = p.height / R; a.w = p.width / R;
  const long long hw = (long long)a.h * a.w;
  const bool v4 = p.width % 4 == 0 && aligned_to(d_depth_in, 16) && aligned_to(d_depth_out, 16);
  const int tile_w = v4 ? 64 : 16;
  const long long tiles_x = ((long long)p.width + tile_w - 1) / tile_w, tiles_y = ((long long)p.height + RV_DN_TILE_ROWS - 1) / RV_DN_TILE_ROWS;
  const long long blocks = (long long)w->n * tiles_x * tiles_y;
  const long long q = (hw + 3) / 4, total = (long long)w->n * q;
  if (blocks > 0x7fffffffLL || (total + 255) / 256 > 0x7fffffffLL)
    return fail(RV_ERR_VALUE, "rv_depth_noise: too many pixels for one launch");
  a.Q = (int)q;
  const size_t need = 2 * (size_t)w->n + (d_grid ? 0 : (size_t)w->n * (size_t)hw);
  int rc = ensure_floats(w, &w->d_dn_scratch, &w->dn_scratch_cap, need); if (rc != RV_OK) return rc;
  a.g = w->d_dn_scratch; a.flag = reinterpret_cast<uint32_t*>(w->d_dn_scratch + w->n);
  a.grid = d_grid ? d_grid : w->d_dn_scratch + 2 * (size_t)w->n;
  hipLaunchKernelGGL(k_depth_noise_draw, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, w->stream, w->d_cfg, a, total);
  HIPCHK(hipGetLastError());
  if (v4) hipLaunchKernelGGL(k_depth_noise_apply<4>, dim3((unsigned)blocks), dim3(256), 0, w->stream, a, (int)tiles_x, (int)tiles_y);
  else hipLaunchKernelGGL(k_depth_noise_apply<1>, dim3((unsigned)blocks), dim3(256), 0, w->stream, a, (int)tiles_x, (int)tiles_y);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
static int seg_env_range(const rv_world* w, const char* who, int32_t env_first, int32_t env_count) {
  if (env_first < 0 || env_count < 1 || (long long)env_first + env_count > (long long)w->n)
    return fail(RV_ERR_VALUE, std::string(who) + ": envs env_first .. env_first + env_count - 1 must lie in [0, N) and be at least one");
  return RV_OK;
}
int rv_deproject(rv_world* w, int32_t env_first, int32_t env_count, const float* d_depth, float* d_points, uint8_t* d_valid) {
  WCHK(w);
  NEED(d_depth, "rv_deproject"); NEED(d_points, "rv_deproject"); NEED(d_valid, "rv_deproject");
  if (!aligned_to(d_depth, 4) || !aligned_to(d_points, 4)) return fail(RV_ERR_VALUE, "rv_deproject: the float buffers must be 4-byte aligned");
  int rc = seg_env_range(w, "rv_deproject", env_first, env_count); if (rc != RV_OK) return rc;
  rc = ensure_snaps(w, (size_t)w->n); if (rc != RV_OK) return rc;
  SIMPLE_LAUNCH(k_obs_snap, w->d_envs, w->n, w->d_snaps, w->d_scene);
  const size_t total = (size_t)env_count * w->cfg.cam_height * w->cfg.cam_width;
  if ((total + 255) / 256 > 0x7fffffffULL) return fail(RV_ERR_VALUE, "rv_deproject: too many pixels for one launch");
  hipLaunchKernelGGL(k_deproject, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, w->stream, w->d_snaps, (int)env_first, total,
                     d_depth, d_points, d_valid, w->d_cfg);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_segment_cloud(rv_world* w, const rv_segment_params* h_params, int32_t env_first, int32_t env_count, const float* d_points,
                     const uint8_t* d_valid, int32_t m, int32_t* d_labels, float* d_clouds, int32_t* d_slot_labels,
                     int32_t* d_slot_counts, float* d_plane, int32_t* d_info) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_segment_cloud: null params");
  NEED(d_points, "rv_segment_cloud"); NEED(d_labels, "rv_segment_cloud"); NEED(d_clouds, "rv_segment_cloud");
  NEED(d_slot_labels, "rv_segment_cloud"); NEED(d_slot_counts, "rv_segment_cloud"); NEED(d_plane, "rv_segment_cloud"); NEED(d_info, "rv_segment_cloud");
  if (!aligned_to(d_points, 4) || !aligned_to(d_labels, 4) || !aligned_to(d_clouds, 4) || !aligned_to(d_slot_labels, 4) ||
      !aligned_to(d_slot_counts, 4) || !aligned_to(d_plane, 4) || !aligned_to(d_info, 4))
    return fail(RV_ERR_VALUE, "rv_segment_cloud: the buffers must be 4-byte aligned");
  const rv_segment_params& p = *h_params;
  int rc = seg_env_range(w, "rv_segment_cloud", env_first, env_count); if (rc != RV_OK) return rc;
  if (m < 1 || m > (1 << 24)) return fail(RV_ERR_VALUE, "rv_segment_cloud: M outside [1, 2^24]");
  if (p.num_hypotheses < 0 || p.num_hypotheses > RV_SEG_MAX_HYPOTHESES) return fail(RV_ERR_VALUE, "rv_segment_cloud: num_hypotheses outside [0, RV_SEG_MAX_HYPOTHESES]");
  if (p.num_clusters < 1 || p.num_clusters > RV_SEG_MAXSLOTS) return fail(RV_ERR_VALUE, "rv_segment_cloud: num_clusters outside [1, RV_SEG_MAXSLOTS]");
  if (p.num_points < 1 || p.num_points > RV_SEG_MAX_POINTS) return fail(RV_ERR_VALUE, "rv_segment_cloud: num_points outside [1, 65536]");
  if (!(p.eps > 0.0f) || !(p.eps - p.eps == 0.0f)) return fail(RV_ERR_VALUE, "rv_segment_cloud: eps must be positive and finite");
  if (!(p.plane_thresh > 0.0f) || !(p.plane_thresh - p.plane_thresh == 0.0f)) return fail(RV_ERR_VALUE, "rv_segment_cloud: plane_thresh must be positive and finite");
  if (p.min_samples < 1) return fail(RV_ERR_VALUE, "rv_segment_cloud: min_samples < 1");
  if (p.draw_index < 0 || p.draw_index > 0xffffffffLL) return fail(RV_ERR_VALUE, "rv_segment_cloud: draw_index outside [0, 2^32)");
  rc = ensure_floats(w, &w->d_seg_scratch, &w->seg_scratch_cap, (size_t)env_count * (size_t)m); if (rc != RV_OK) return rc;
  SegArgs a;
  a.p = p; a.pts = d_points; a.valid = d_valid; a.M = m; a.env_first = env_first;
  a.labels = d_labels; a.clouds = d_clouds; a.slot_labels = d_slot_labels; a.slot_counts = d_slot_counts; a.plane = d_plane; a.info = d_info;
  a.idx = reinterpret_cast<int32_t*>(w->d_seg_scratch);
  hipLaunchKernelGGL(k_segment_cloud, dim3((unsigned)env_count), dim3(RV_SEG_THREADS), 0, w->stream, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
size_t rv_ward_workspace_bytes(int32_t env_count) { return env_count < 1 ? 0 : (size_t)env_count * RV_WARD_ENV_BYTES; }
int rv_ward_groups(rv_world* w, const rv_ward_params* h_params, int32_t env_first, int32_t env_count, const float* d_points,
                   const int32_t* d_labels, int32_t m, void* d_workspace, size_t workspace_bytes, int32_t* d_groups, float* d_clouds,
                   int32_t* d_slot_counts, int32_t* d_info) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_ward_groups: null params");
  NEED(d_points, "rv_ward_groups"); NEED(d_labels, "rv_ward_groups"); NEED(d_workspace, "rv_ward_groups"); NEED(d_groups, "rv_ward_groups");
  NEED(d_clouds, "rv_ward_groups"); NEED(d_slot_counts, "rv_ward_groups"); NEED(d_info, "rv_ward_groups");
  if (!aligned_to(d_points, 4) || !aligned_to(d_labels, 4) || !aligned_to(d_groups, 4) || !aligned_to(d_clouds, 4) ||
      !aligned_to(d_slot_counts, 4) || !aligned_to(d_info, 4))
    return fail(RV_ERR_VALUE, "rv_ward_groups: the buffers must be 4-byte aligned");
  if (!aligned_to(d_workspace, 8)) return fail(RV_ERR_VALUE, "rv_ward_groups: the workspace must be 8-byte aligned");
  const rv_ward_params& p = *h_params;
  int rc = seg_env_range(w, "rv_ward_groups", env_first, env_count); if (rc != RV_OK) return rc;
  if (workspace_bytes < rv_ward_workspace_bytes(env_count)) return fail(RV_ERR_VALUE, "rv_ward_groups: the workspace is smaller than rv_ward_workspace_bytes(env_count)");
  if (m < 1 || m > (1 << 24)) return fail(RV_ERR_VALUE, "rv_ward_groups: M outside [1, 2^24]");
  if (p.num_neighbors < 1 || p.num_neighbors > RV_WARD_MAX_NEIGHBORS) return fail(RV_ERR_VALUE, "rv_ward_groups: num_neighbors outside [1, RV_WARD_MAX_NEIGHBORS]");
  if (p.num_groups < 1 || p.num_groups > RV_SEG_MAXSLOTS) return fail(RV_ERR_VALUE, "rv_ward_groups: num_groups outside [1, RV_SEG_MAXSLOTS]");
  if (p.num_points < 1 || p.num_points > RV_SEG_MAX_POINTS) return fail(RV_ERR_VALUE, "rv_ward_groups: num_points outside [1, 65536]");
  if (p.draw_index < 0 || p.draw_index > 0xffffffffLL) return fail(RV_ERR_VALUE, "rv_ward_groups: draw_index outside [0, 2^32)");
  WardArgs a;
  a.p = p; a.pts = d_points; a.labels = d_labels; a.M = m; a.env_first = env_first;
  a.adj = reinterpret_cast<unsigned long long*>(d_workspace);
  a.idx = reinterpret_cast<int32_t*>(a.adj + (size_t)env_count * RV_WARD_MAXPTS * RV_WARD_ROW_WORDS);
  a.groups = d_groups; a.clouds = d_clouds; a.slot_counts = d_slot_counts; a.info = d_info;
  hipLaunchKernelGGL(k_ward_groups, dim3((unsigned)env_count), dim3(RV_WARD_THREADS), 0, w->stream, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_grasp_crops(rv_world* w, const rv_grasp_crop_params* h_params, const float* d_depth, const float* d_grasps, int32_t k,
                   float* d_images, float* d_grasp_depths) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_grasp_crops: null params");
  NEED(d_depth, "rv_grasp_crops"); NEED(d_grasps, "rv_grasp_crops"); NEED(d_images, "rv_grasp_crops");
  const rv_grasp_crop_params& p = *h_params;
  if (!aligned_to(d_depth, 4) || !aligned_to(d_grasps, 4) || !aligned_to(d_images, 4) || !aligned_to(d_grasp_depths, 4))
    return fail(RV_ERR_VALUE, "rv_grasp_crops: the buffers must be 4-byte aligned");
  if (p.height < 1 || p.width < 1) return fail(RV_ERR_VALUE, "rv_grasp_crops: height or width < 1");
  if (p.crop_height < 1 || p.crop_height > RV_GC_MAX_SIDE || p.crop_width < 1 || p.crop_width > RV_GC_MAX_SIDE)
    return fail(RV_ERR_VALUE, "rv_grasp_crops: crop_height or crop_width outside [1, RV_GC_MAX_SIDE]");
  if (p.step < 1 || p.step > RV_GC_MAX_STEP) return fail(RV_ERR_VALUE, "rv_grasp_crops: step outside [1, RV_GC_MAX_STEP]");
  if (k < 1 || k > RV_AP_MAX_SAMPLES) return fail(RV_ERR_VALUE, "rv_grasp_crops: k outside [1, RV_AP_MAX_SAMPLES]");
  const long long rows = (long long)w->n * k;
  const int px = p.crop_height * p.crop_width;
  // a wave owns 64 P consecutive pixels of one image: P = 4 (16-byte stores) when the images allow it
  const bool v4 = px % 4 == 0 && px >= 256 && aligned_to(d_images, 16);
  const int per_wave = v4 ? 256 : 64;
  const long long units = (px + per_wave - 1) / per_wave, waves = rows * units;
  if (rows > 0x7fffffffLL || waves > 0x7fffffffLL) return fail(RV_ERR_VALUE, "rv_grasp_crops: too many pixels for one launch");
  GcArgs a;
  a.depth = d_depth; a.grasps = d_grasps; a.images = d_images; a.grasp_depths = d_grasp_depths;
  a.H = p.height; a.W = p.width; a.h = p.crop_height; a.w = p.crop_width; a.step = p.step;
  a.units = (uint32_t)units; a.rows = (uint32_t)rows; a.K = (uint32_t)k;
  const dim3 grid((unsigned)((waves + 3) / 4));
  if (v4) hipLaunchKernelGGL(k_grasp_crops<4>, grid, dim3(256), 0, w->stream, a);
  else hipLaunchKernelGGL(k_grasp_crops<1>, grid, dim3(256), 0, w->stream, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
static bool gq_model_ok(const rv_grasp_quality_model& m) {
  const auto side = [](int v) { return v >= RV_GQ_MIN_SIDE && v <= RV_GQ_MAX_SIDE && v % 4 == 0; };
  const auto mult4 = [](int v, int hi) { return v >= 4 && v <= hi && v % 4 == 0; };
  return side(m.height) && side(m.width) && mult4(m.c1, RV_GQ_MAX_CHANNELS) && mult4(m.c2, RV_GQ_MAX_CHANNELS) &&
         mult4(m.f1, RV_GQ_MAX_FEATURES) && mult4(m.f2, RV_GQ_MAX_FEATURES) && mult4(m.p, RV_GQ_MAX_POSE) && m.reserved == 0;
}
int64_t rv_grasp_quality_weight_count(const rv_grasp_quality_model* h_model) {
  if (!h_model || !gq_model_ok(*h_model)) return -1;
  const rv_grasp_quality_model& m = *h_model;
  return (int64_t)gq_layout(m.height, m.width, m.c1, m.c2, m.f1, m.f2, m.p).count;
}
int rv_grasp_quality(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                     const float* d_images, const float* d_grasp_depths, int32_t k, float* d_logits) {
  WCHK(w);
  if (!h_model) return fail(RV_ERR_VALUE, "rv_grasp_quality: null model");
  NEED(d_weights, "rv_grasp_quality"); NEED(d_images, "rv_grasp_quality"); NEED(d_grasp_depths, "rv_grasp_quality");
  NEED(d_logits, "rv_grasp_quality");
  const rv_grasp_quality_model& m = *h_model;
  if (!aligned_to(d_weights, 4) || !aligned_to(d_images, 4) || !aligned_to(d_grasp_depths, 4) || !aligned_to(d_logits, 4))
    return fail(RV_ERR_VALUE, "rv_grasp_quality: the buffers must be 4-byte aligned");
  if (!gq_model_ok(m)) return fail(RV_ERR_VALUE, "rv_grasp_quality: a size of the model is outside its range");
  const float big = 3.402823466e38f;
  const auto finite = [big](float v) { return v >= -big && v <= big; };
  if (!finite(m.im_mean) || !finite(m.im_inv_std) || !finite(m.z_mean) || !finite(m.z_inv_std))
    return fail(RV_ERR_VALUE, "rv_grasp_quality: a normalisation constant is not finite");
  if (k < 1 || k > RV_AP_MAX_SAMPLES) return fail(RV_ERR_VALUE, "rv_grasp_quality: k outside [1, RV_AP_MAX_SAMPLES]");
  const long long rows = (long long)w->n * k;
  if (rows > 0x7fffffffLL) return fail(RV_ERR_VALUE, "rv_grasp_quality: too many samples for one launch");
  const GqLayout L = gq_layout(m.height, m.width, m.c1, m.c2, m.f1, m.f2, m.p);
  const size_t lds = (size_t)L.l_floats * sizeof(float);
  // (more than the 64 KB a kernel gets unasked; 78 KB for the largest model, two workgroups per CU)
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_grasp_quality), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  GqArgs a;
  a.images = d_images; a.depths = d_grasp_depths; a.logits = d_logits;
  a.h = m.height; a.w = m.width; a.c1 = m.c1; a.c2 = m.c2; a.f1 = m.f1; a.f2 = m.f2; a.p = m.p;
  a.im_mean = m.im_mean; a.im_inv_std = m.im_inv_std; a.z_mean = m.z_mean; a.z_inv_std = m.z_inv_std;
  a.rows = (uint32_t)rows;
  const dim3 grid((unsigned)((rows + RV_GQ_BATCH - 1) / RV_GQ_BATCH));
  hipLaunchKernelGGL(k_grasp_quality, grid, dim3(RV_GQ_TPB), lds, w->stream, a, d_weights);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
// -- a training step of the grasp-quality network (rv_dev_grasp_train.h)
static bool gq_norm_finite(const rv_grasp_quality_model& m) {
  const float big = 3.402823466e38f;
  const auto finite = [big](float v) { return v >= -big && v <= big; };
  return finite(m.im_mean) && finite(m.im_inv_std) && finite(m.z_mean) && finite(m.z_inv_std);
}
static bool ranges_overlap(const void* a, size_t abytes, const void* b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}
static GtArgs gt_args(const rv_grasp_quality_model& m, int64_t rows) {
  GtArgs a;
  a.images = nullptr; a.depths = nullptr; a.dlogits = nullptr; a.ws = nullptr; a.logits = nullptr; a.grad = nullptr;
  a.h = m.height; a.w = m.width; a.c1 = m.c1; a.c2 = m.c2; a.f1 = m.f1; a.f2 = m.f2; a.p = m.p;
  a.im_mean = m.im_mean; a.im_inv_std = m.im_inv_std; a.z_mean = m.z_mean; a.z_inv_std = m.z_inv_std;
  a.rows = (uint32_t)rows;
  return a;
}
int64_t rv_grasp_quality_train_workspace_floats(const rv_grasp_quality_model* h_model, int64_t m) {
  if (!h_model || !gq_model_ok(*h_model) || m < 1 || m > RV_GQ_MAX_BATCH) return -1;
  const rv_grasp_quality_model& q = *h_model;
  return m * (int64_t)gt_layout(q.height, q.width, q.c1, q.c2, q.f1, q.f2, q.p).stride;
}
int rv_grasp_quality_forward_train(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                                   const float* d_images, const float* d_grasp_depths, int64_t m,
                                   float* d_workspace, float* d_logits) {
  WCHK(w);
  if (!h_model) return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: null model");
  NEED(d_weights, "rv_grasp_quality_forward_train"); NEED(d_images, "rv_grasp_quality_forward_train");
  NEED(d_grasp_depths, "rv_grasp_quality_forward_train"); NEED(d_workspace, "rv_grasp_quality_forward_train");
  NEED(d_logits, "rv_grasp_quality_forward_train");
  const rv_grasp_quality_model& q = *h_model;
  if (!aligned_to(d_weights, 4) || !aligned_to(d_images, 4) || !aligned_to(d_grasp_depths, 4) || !aligned_to(d_workspace, 4) ||
      !aligned_to(d_logits, 4))
    return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: the buffers must be 4-byte aligned");
  if (!gq_model_ok(q)) return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: a size of the model is outside its range");
  if (!gq_norm_finite(q)) return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: a normalisation constant is not finite");
  if (m < 1 || m > RV_GQ_MAX_BATCH) return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: m outside [1, RV_GQ_MAX_BATCH]");
  const GqLayout L = gq_layout(q.height, q.width, q.c1, q.c2, q.f1, q.f2, q.p);
  const GtLayout T = gt_layout(q.height, q.width, q.c1, q.c2, q.f1, q.f2, q.p);
  const size_t wsb = (size_t)m * (size_t)T.stride * sizeof(float);
  if (ranges_overlap(d_workspace, wsb, d_logits, (size_t)m * sizeof(float)) ||
      ranges_overlap(d_workspace, wsb, d_weights, (size_t)L.count * sizeof(float)) ||
      ranges_overlap(d_logits, (size_t)m * sizeof(float), d_weights, (size_t)L.count * sizeof(float)))
    return fail(RV_ERR_VALUE, "rv_grasp_quality_forward_train: d_workspace, d_logits and d_weights must not overlap");
  const size_t lds = (size_t)L.l_floats * sizeof(float);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gq_train_forward), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  GtArgs a = gt_args(q, m);
  a.images = d_images; a.depths = d_grasp_depths; a.ws = d_workspace; a.logits = d_logits;
  const dim3 grid((unsigned)((m + RV_GQ_BATCH - 1) / RV_GQ_BATCH));
  hipLaunchKernelGGL(k_gq_train_forward, grid, dim3(RV_GQ_TPB), lds, w->stream, a, d_weights);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_grasp_quality_backward(rv_world* w, const rv_grasp_quality_model* h_model, const float* d_weights,
                              const float* d_images, const float* d_grasp_depths, const float* d_dlogits, int64_t m,
                              float* d_workspace, float* d_grad) {
  WCHK(w);
  if (!h_model) return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: null model");
  NEED(d_weights, "rv_grasp_quality_backward"); NEED(d_images, "rv_grasp_quality_backward");
  NEED(d_grasp_depths, "rv_grasp_quality_backward"); NEED(d_dlogits, "rv_grasp_quality_backward");
  NEED(d_workspace, "rv_grasp_quality_backward"); NEED(d_grad, "rv_grasp_quality_backward");
  const rv_grasp_quality_model& q = *h_model;
  if (!aligned_to(d_weights, 4) || !aligned_to(d_images, 4) || !aligned_to(d_grasp_depths, 4) || !aligned_to(d_dlogits, 4) ||
      !aligned_to(d_workspace, 4) || !aligned_to(d_grad, 4))
    return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: the buffers must be 4-byte aligned");
  if (!gq_model_ok(q)) return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: a size of the model is outside its range");
  if (!gq_norm_finite(q)) return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: a normalisation constant is not finite");
  if (m < 1 || m > RV_GQ_MAX_BATCH) return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: m outside [1, RV_GQ_MAX_BATCH]");
  const GqLayout L = gq_layout(q.height, q.width, q.c1, q.c2, q.f1, q.f2, q.p);
  const GtLayout T = gt_layout(q.height, q.width, q.c1, q.c2, q.f1, q.f2, q.p);
  const size_t gb = (size_t)L.count * sizeof(float), mb = (size_t)m * sizeof(float);
  if (ranges_overlap(d_grad, gb, d_weights, gb) || ranges_overlap(d_grad, gb, d_images, mb * (size_t)(q.height * q.width)) ||
      ranges_overlap(d_grad, gb, d_grasp_depths, mb) || ranges_overlap(d_grad, gb, d_dlogits, mb) ||
      ranges_overlap(d_grad, gb, d_workspace, mb * (size_t)T.stride))
    return fail(RV_ERR_VALUE, "rv_grasp_quality_backward: d_grad must not overlap an input or the workspace");
  const size_t lds = (size_t)T.l_floats * sizeof(float);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gq_train_backward_sample), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  GtArgs a = gt_args(q, m);
  a.images = d_images; a.depths = d_grasp_depths; a.dlogits = d_dlogits; a.ws = d_workspace; a.grad = d_grad;
  hipLaunchKernelGGL(k_gq_train_backward_sample, dim3((unsigned)m), dim3(RV_GT_TPB), lds, w->stream, a, d_weights);
  HIPCHK(hipGetLastError());
  const dim3 grid((unsigned)((L.count + RV_GT_TPB - 1) / RV_GT_TPB));
  hipLaunchKernelGGL(k_gq_train_backward_weights, grid, dim3(RV_GT_TPB), 0, w->stream, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_adam_step(rv_world* w, const rv_adam_params* h_params, int64_t count, float* d_w, const float* d_g, float* d_m, float* d_v) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_adam_step: null params");
  NEED(d_w, "rv_adam_step"); NEED(d_g, "rv_adam_step"); NEED(d_m, "rv_adam_step"); NEED(d_v, "rv_adam_step");
  if (!aligned_to(d_w, 4) || !aligned_to(d_g, 4) || !aligned_to(d_m, 4) || !aligned_to(d_v, 4))
    return fail(RV_ERR_VALUE, "rv_adam_step: the buffers must be 4-byte aligned");
  if (count < 1 || count > ((int64_t)0x7fffffff) * RV_GT_TPB) return fail(RV_ERR_VALUE, "rv_adam_step: count < 1 or too large for one launch");
  const rv_adam_params& p = *h_params;
  const float big = 3.402823466e38f;
  const auto finite = [big](float v) { return v >= -big && v <= big; };
  if (!finite(p.lr) || !finite(p.beta1) || !finite(p.beta2) || !finite(p.eps) || !finite(p.corr1) || !finite(p.corr2))
    return fail(RV_ERR_VALUE, "rv_adam_step: a parameter is not finite");
  if (!(p.beta1 >= 0.0f && p.beta1 < 1.0f) || !(p.beta2 >= 0.0f && p.beta2 < 1.0f))
    return fail(RV_ERR_VALUE, "rv_adam_step: beta1 or beta2 outside [0, 1)");
  if (p.reserved[0] != 0 || p.reserved[1] != 0) return fail(RV_ERR_VALUE, "rv_adam_step: a reserved word is not 0");
  const size_t bytes = (size_t)count * sizeof(float);
  if (ranges_overlap(d_w, bytes, d_g, bytes) || ranges_overlap(d_w, bytes, d_m, bytes) || ranges_overlap(d_w, bytes, d_v, bytes) ||
      ranges_overlap(d_g, bytes, d_m, bytes) || ranges_overlap(d_g, bytes, d_v, bytes) || ranges_overlap(d_m, bytes, d_v, bytes))
    return fail(RV_ERR_VALUE, "rv_adam_step: the four buffers must not overlap");
  GtAdam a;
  a.lr = p.lr; a.beta1 = p.beta1; a.beta2 = p.beta2; a.eps = p.eps; a.corr1 = p.corr1; a.corr2 = p.corr2;
  const dim3 grid((unsigned)((count + RV_GT_TPB - 1) / RV_GT_TPB));
  hipLaunchKernelGGL(k_adam_step, grid, dim3(RV_GT_TPB), 0, w->stream, a, (size_t)count, d_w, d_g, d_m, d_v);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_grasp_refine(rv_world* w, const rv_grasp_refine_params* h_params, const rv_antipodal_params* h_sampler,
                    const float* d_depth, const float* d_grasps, const float* d_scores, const int32_t* d_count,
                    const int32_t* d_status, int32_t k, float* d_grasps_out, float* d_actions4_out,
                    int32_t* d_parent, int32_t* d_count_out) {
  WCHK(w);
  if (!h_params || !h_sampler) return fail(RV_ERR_VALUE, "rv_grasp_refine: null params");
  NEED(d_depth, "rv_grasp_refine"); NEED(d_grasps, "rv_grasp_refine"); NEED(d_scores, "rv_grasp_refine");
  NEED(d_grasps_out, "rv_grasp_refine");
  const rv_grasp_refine_params& p = *h_params;
  if (!aligned_to(d_depth, 4) || !aligned_to(d_grasps, 4) || !aligned_to(d_scores, 4) || !aligned_to(d_count, 4) ||
      !aligned_to(d_status, 4) || !aligned_to(d_grasps_out, 4) || !aligned_to(d_actions4_out, 4) || !aligned_to(d_parent, 4) ||
      !aligned_to(d_count_out, 4))
    return fail(RV_ERR_VALUE, "rv_grasp_refine: the buffers must be 4-byte aligned");
  if (d_grasps_out == d_grasps) return fail(RV_ERR_VALUE, "rv_grasp_refine: d_grasps_out must not be d_grasps");
  if (k < 1 || k > RV_AP_MAX_SAMPLES) return fail(RV_ERR_VALUE, "rv_grasp_refine: k outside [1, RV_AP_MAX_SAMPLES]");
  if (p.n_elites < 1 || p.n_elites > k) return fail(RV_ERR_VALUE, "rv_grasp_refine: n_elites outside [1, k]");
  if (p.height < 1 || p.width < 1) return fail(RV_ERR_VALUE, "rv_grasp_refine: height or width < 1");
  const float big = 3.402823466e38f;
  const auto sigma_ok = [big](float v) { return v >= 0.0f && v <= big; };
  if (!sigma_ok(p.sigma_center) || !sigma_ok(p.sigma_angle) || !sigma_ok(p.sigma_depth))
    return fail(RV_ERR_VALUE, "rv_grasp_refine: a sigma is negative or not finite");
  if (p.macro_index < 0 || p.macro_index >= RV_GR_MAX_MACRO_INDEX) return fail(RV_ERR_VALUE, "rv_grasp_refine: macro_index outside [0, 2^24)");
  if (p.iteration < 0 || p.iteration >= RV_GR_MAX_ITERATION) return fail(RV_ERR_VALUE, "rv_grasp_refine: iteration outside [0, 2^26)");
  if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return fail(RV_ERR_VALUE, "rv_grasp_refine: a reserved word is not zero");
  if (d_actions4_out && w->cfg.env_type != RV_ENV_GRASP) return fail(RV_ERR_VALUE, "rv_grasp_refine: d_actions4_out needs a Grasp4DofEnv world");
  GrArgs a;
  int rc = antipodal_geometry(*h_sampler, p.height, p.width, "rv_grasp_refine", &a.ap); if (rc != RV_OK) return rc;
  a.ap.depth = d_depth;
  a.p = p; a.grasps = d_grasps; a.scores = d_scores; a.count = d_count; a.status = d_status;
  a.grasps_out = d_grasps_out; a.actions4 = d_actions4_out; a.parent = d_parent; a.count_out = d_count_out; a.K = k;
  // one wave per env, four envs per workgroup
  const int per = RV_GR_TPB / 64;
  hipLaunchKernelGGL(k_grasp_refine, dim3((unsigned)((w->n + per - 1) / per)), dim3(RV_GR_TPB), 0, w->stream, w->d_envs, w->n, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int64_t rv_state_bytes(const rv_world* w) { (void)w; return (int64_t)sizeof(DevEnv); }
int rv_state_save(rv_world* w, void* d_buf) {
  WCHK(w); NEED(d_buf, "rv_state_save");
  if (!aligned_to(d_buf, 4)) return fail(RV_ERR_VALUE, "rv_state_save: the buffer must be 4-byte aligned");
  if (state_identity_by_runtime()) { HIPCHK(hipMemcpyAsync(d_buf, w->d_envs, sizeof(DevEnv) * (size_t)w->n, hipMemcpyDeviceToDevice, w->stream)); return RV_OK; }
  return launch_gather(w->stream, d_buf, w->d_envs, w->n, w->n, nullptr, 1);
}
int rv_state_load(rv_world* w, const void* d_buf, int32_t n_blocks, const int32_t* d_index) {
  WCHK(w); NEED(d_buf, "rv_state_load");
  if (!aligned_to(d_buf, 4) || !aligned_to(d_index, 4)) return fail(RV_ERR_VALUE, "rv_state_load: the buffers must be 4-byte aligned");
  if (n_blocks < 1) return fail(RV_ERR_VALUE, "rv_state_load: n_blocks must be positive");
  if (!d_index && n_blocks != w->n) return fail(RV_ERR_VALUE, "rv_state_load: without an index the buffer must hold one block per env");
  if (!d_index && state_identity_by_runtime()) { HIPCHK(hipMemcpyAsync(w->d_envs, d_buf, sizeof(DevEnv) * (size_t)w->n, hipMemcpyDeviceToDevice, w->stream)); return RV_OK; }
  return launch_gather(w->stream, w->d_envs, d_buf, w->n, n_blocks, d_index, 1);
}
int rv_branch(rv_world* dst, rv_world* src, int32_t s) {
  WCHK(src); WCHK(dst);
  int rc = branch_check(dst, src, s, "rv_branch"); if (rc != RV_OK) return rc;
  return branch_copy(dst, src, s);
}
// the tail of rv_plan_simulate, rv_plan_propose and rv_plan_propose_route, after the caller's own checks: the launch
// limit, the branch copy, then h x (before(t) -- what fills slice t of d_actions, if anything --, the slice into the envs,
// one env.step(), the optional record)
struct plan_no_before { int operator()(int) const { return RV_OK; } };
extern "C++" template <class Before = plan_no_before>
static int plan_steps(rv_world* w, rv_world* src, int s, int h, const float* d_actions, float* d_states, float* d_rewards,
                      uint8_t* d_dones, const std::string& me, Before before = Before()) {
  const int G = w->cfg.num_goal_steps > 0 ? w->cfg.num_goal_steps : 1;
  if ((long long)w->n * G * 4 > 0x7fffffffLL || (long long)w->n * RV_MAXB > 0x7fffffffLL) return fail(RV_ERR_VALUE, me + ": too many envs for one launch");
  int rc = branch_copy(w, src, s); if (rc != RV_OK) return rc;
  for (int t = 0; t < h; ++t) {
    rc = before(t); if (rc != RV_OK) return rc;
    hipLaunchKernelGGL(k_plan_actions, dim3((unsigned)((w->n * G * 4 + 255) / 256)), dim3(256), 0, w->stream, w->d_envs, w->n, d_actions, G, h, t);
    HIPCHK(hipGetLastError());
    rc = launch_env<MODE_MACRO>(w, nullptr, 0, 0, 0, 0, 0, 0); if (rc != RV_OK) return rc;
    if (d_states || d_rewards || d_dones) {
      hipLaunchKernelGGL(k_plan_record, dim3((unsigned)((w->n * RV_MAXB + 255) / 256)), dim3(256), 0, w->stream, w->d_envs, w->n, h, t, d_states, d_rewards, d_dones);
      HIPCHK(hipGetLastError());
    }
  }
  return RV_OK;
}
int rv_plan_simulate(rv_world* plan, rv_world* src, const float* d_actions, int32_t s, int32_t h,
                     float* d_states, float* d_rewards, uint8_t* d_dones) {
  WCHK(src); WCHK(plan);
  if (src->cfg.env_type == RV_ENV_GRASP || plan->cfg.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, "rv_plan_simulate: PushEnv worlds only");
  int rc = branch_check(plan, src, s, "rv_plan_simulate"); if (rc != RV_OK) return rc;
  if (h < 1) return fail(RV_ERR_VALUE, "rv_plan_simulate: h must be positive");
  NEED(d_actions, "rv_plan_simulate");
  if (!aligned_to(d_actions, 4) || !aligned_to(d_states, 8) || !aligned_to(d_rewards, 4)) return fail(RV_ERR_VALUE, "rv_plan_simulate: the states must be 8-byte aligned, actions and rewards 4-byte aligned");
  return plan_steps(plan, src, s, h, d_actions, d_states, d_rewards, d_dones, "rv_plan_simulate");
}
// the range checks hp_check and pr_check share: s, copies, env_id_offset % copies, max_attempts, plan_index, step, the
// launch limit
static int proposal_range_check(const rv_world* w, int32_t s, int32_t copies, int32_t max_attempts, int32_t plan_index, int32_t step, const std::string& me) {
  if (s < 1 || s > RV_HP_MAX_SAMPLES) return fail(RV_ERR_VALUE, me + ": s outside [1, RV_HP_MAX_SAMPLES]");
  if (copies < 1 || (long long)copies * s > RV_HP_MAX_SAMPLES) return fail(RV_ERR_VALUE, me + ": copies < 1 or copies * s > RV_HP_MAX_SAMPLES");
  if (w->cfg.env_id_offset % copies != 0) return fail(RV_ERR_VALUE, me + ": env_id_offset is not a multiple of copies");
  if (max_attempts < 1 || max_attempts > RV_HP_MAX_ATTEMPTS) return fail(RV_ERR_VALUE, me + ": max_attempts outside [1, RV_HP_MAX_ATTEMPTS]");
  if (plan_index < 0 || plan_index >= RV_HP_MAX_PLAN_INDEX) return fail(RV_ERR_VALUE, me + ": plan_index outside [0, 2^24)");
  if (step < 0 || step >= RV_HP_MAX_STEP) return fail(RV_ERR_VALUE, me + ": step outside [0, 64)");
  if ((long long)w->n * s > 0x7fffffffLL) return fail(RV_ERR_VALUE, me + ": too many candidates for one launch");
  return RV_OK;
}
// the checks rv_policy_heuristic_multi and rv_plan_propose share: `w` is the world the kernel reads, p the params it is
// launched with (rv_plan_propose: copies already x s, step the last one), s the candidates per env of w
static int hp_check(const rv_world* w, const rv_push_proposal_params& p, int32_t s, const std::string& me) {
  if (w->cfg.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, me + ": a PushEnv world only");
  if (p.mode != RV_HP_EPISODE && p.mode != RV_HP_SPREAD) return fail(RV_ERR_VALUE, me + ": unknown mode");
  int rc = proposal_range_check(w, s, p.copies, p.max_attempts, p.plan_index, p.step, me); if (rc != RV_OK) return rc;
  if (p.mode == RV_HP_EPISODE && (p.plan_index != 0 || p.step != 0 || p.seed != 0u || p.copies != 1))
    return fail(RV_ERR_VALUE, me + ": RV_HP_EPISODE takes plan_index, step and seed 0 and copies 1");
  if (!(p.start_margin >= 0.0f) || !(p.motion_margin >= 0.0f)) return fail(RV_ERR_VALUE, me + ": a margin is negative or NaN");
  return RV_OK;
}
// rows of (env, candidate) are (m * s + k) * h + t (csrc/rv_dev_push_sampler.h)
static int hp_launch(rv_world* w, const rv_push_proposal_params& p, int s, int h, int t, float* d_actions, int32_t* d_status) {
  HpArgs a;
  a.p = p; a.actions = d_actions; a.status = d_status; a.S = s; a.h = h; a.t = t;
  if (p.mode == RV_HP_EPISODE) {
    hipLaunchKernelGGL(k_push_proposals_episode, dim3((unsigned)w->n), dim3(64), 0, w->stream, w->d_envs, w->n, w->d_cfg, a);
  } else {
    const long long waves = (long long)w->n * s;
    hipLaunchKernelGGL(k_push_proposals_spread, dim3((unsigned)((waves + RV_HP_WAVES - 1) / RV_HP_WAVES)), dim3(64 * RV_HP_WAVES), 0, w->stream,
                       w->d_envs, w->n, w->d_cfg, a);
  }
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_policy_heuristic_multi(rv_world* w, const rv_push_proposal_params* h_params, int32_t s, float* d_actions, int32_t* d_status) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_policy_heuristic_multi: null params");
  int rc = hp_check(w, *h_params, s, "rv_policy_heuristic_multi"); if (rc != RV_OK) return rc;
  NEED(d_actions, "rv_policy_heuristic_multi");
  if (!aligned_to(d_actions, 4) || !aligned_to(d_status, 4)) return fail(RV_ERR_VALUE, "rv_policy_heuristic_multi: the buffers must be 4-byte aligned");
  return hp_launch(w, *h_params, s, 1, 0, d_actions, d_status);
}
// rv_plan_propose and rv_plan_propose_route, the part that does not know the proposal kernel.  Params: the params struct of
// either (both have copies and step); `mode_ok`: what the caller asks of *h_params beyond the ranges; `check(plan, p, 1,
// me)`: the range checks on the params the kernel is launched with (copies already x s, step the last one); `propose(plan,
// p, h, t)`: the launch that writes slice t of d_actions / d_status from the plan world's state, p.step = the step of t
extern "C++" template <class Params, class ModeOk, class Check, class Propose>
static int plan_propose_run(rv_world* plan, rv_world* src, const Params* h_params, int32_t s, int32_t h, float* d_actions, float* d_states,
                            float* d_rewards, uint8_t* d_dones, int32_t* d_status, const char* who, ModeOk mode_ok, Check check, Propose propose) {
  WCHK(src); WCHK(plan);
  const std::string me(who);
  if (src->cfg.env_type == RV_ENV_GRASP || plan->cfg.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, me + ": PushEnv worlds only");
  int rc = branch_check(plan, src, s, who); if (rc != RV_OK) return rc;
  if (h < 1) return fail(RV_ERR_VALUE, me + ": h must be positive");
  if (!h_params) return fail(RV_ERR_VALUE, me + ": null params");
  rc = mode_ok(*h_params); if (rc != RV_OK) return rc;
  if (h_params->copies < 1 || (long long)h_params->copies * s > RV_HP_MAX_SAMPLES) return fail(RV_ERR_VALUE, me + ": copies < 1 or copies * s > RV_HP_MAX_SAMPLES");
  if ((long long)plan->cfg.env_id_offset != (long long)src->cfg.env_id_offset * s) return fail(RV_ERR_VALUE, me + ": the plan world needs env_id_offset = s x the source's");
  // the kernel reads the plan world: one candidate per branch env, copies x s envs per source env, the last step's key
  Params p = *h_params;
  p.copies = h_params->copies * s;
  if (h_params->step < 0 || (long long)h_params->step + h > RV_HP_MAX_STEP) return fail(RV_ERR_VALUE, me + ": step < 0 or step + h > 64");
  p.step = h_params->step + h - 1;
  rc = check(plan, p, 1, me); if (rc != RV_OK) return rc;
  if (!d_actions) return fail(RV_ERR_VALUE, me + ": null buffer");
  if (!aligned_to(d_actions, 4) || !aligned_to(d_states, 8) || !aligned_to(d_rewards, 4) || !aligned_to(d_status, 4))
    return fail(RV_ERR_VALUE, me + ": the states must be 8-byte aligned, actions, rewards and status 4-byte aligned");
  return plan_steps(plan, src, s, h, d_actions, d_states, d_rewards, d_dones, me, [&](int t) {
    p.step = h_params->step + t;
    return propose(plan, p, (int)h, t);
  });
}
int rv_plan_propose(rv_world* plan, rv_world* src, const rv_push_proposal_params* h_params, int32_t s, int32_t h,
                    float* d_actions, float* d_states, float* d_rewards, uint8_t* d_dones, int32_t* d_status) {
  return plan_propose_run(plan, src, h_params, s, h, d_actions, d_states, d_rewards, d_dones, d_status, "rv_plan_propose",
    [](const rv_push_proposal_params& p) { return p.mode == RV_HP_SPREAD ? RV_OK : fail(RV_ERR_VALUE, "rv_plan_propose: the mode must be RV_HP_SPREAD"); },
    hp_check,
    [=](rv_world* w, const rv_push_proposal_params& p, int h_, int t) { return hp_launch(w, p, 1, h_, t, d_actions, d_status); });
}

// ---- route-following push proposals (csrc/rv_dev_push_route.h)
// the config's tiles: what k_route_field and k_push_proposals_route rely on
static int route_cfg_check(const rv_world* w, const std::string& me) {
  const rv_config& c = w->cfg;
  if (c.env_type == RV_ENV_GRASP) return fail(RV_ERR_VALUE, me + ": a PushEnv world only");
  if (c.task != RV_TASK_CROSSING && c.task != RV_TASK_INSERTION) return fail(RV_ERR_VALUE, me + ": the task must be crossing or insertion");
  if (c.n_goal < 1 || c.n_goal > RV_MAXTILES || c.n_region < 0 || c.n_region > RV_MAXTILES) return fail(RV_ERR_VALUE, me + ": n_goal outside [1, RV_MAXTILES] or n_region outside [0, RV_MAXTILES]");
  for (int list = 0; list < 2; ++list) {
    const float (*tiles)[2] = list ? c.goal : c.region;
    const int n = list ? c.n_goal : c.n_region;
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < 2; ++k) {
        const float v = tiles[j][k];
        if (!(v >= 0.0f && v <= (float)(RV_PR_GRID - 1)) || v != (float)(int)v) return fail(RV_ERR_VALUE, me + ": a region or goal tile is no integer pair of the 8 x 8 grid");
      }
  }
  return RV_OK;
}
// the field of a world whose config passed route_cfg_check: made once, on the stream the world has at that moment, and
// waited for -- the world may be given another stream later
static int route_field(rv_world* w) {
  if (w->d_route) return RV_OK;
  uint8_t* d = nullptr;
  HIPCHK(hipMalloc(&d, RV_PR_FIELD_BYTES));
  hipLaunchKernelGGL(k_route_field, dim3(1), dim3(64), 0, w->stream, w->d_cfg, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
  if (e != hipSuccess) { (void)hipFree(d); return fail(RV_ERR_HIP, std::string("k_route_field: ") + hipGetErrorString(e)); }
  w->d_route = d;
  return RV_OK;
}
// the checks rv_policy_route_multi and rv_plan_propose_route share, as hp_check
static int pr_check(const rv_world* w, const rv_push_route_params& p, int32_t s, const std::string& me) {
  int rc = route_cfg_check(w, me); if (rc != RV_OK) return rc;
  rc = proposal_range_check(w, s, p.copies, p.max_attempts, p.plan_index, p.step, me); if (rc != RV_OK) return rc;
  if (!(p.start_margin >= 0.0f) || !(p.angle_jitter >= 0.0f) || !(p.lateral >= 0.0f)) return fail(RV_ERR_VALUE, me + ": start_margin, angle_jitter or lateral is negative or NaN");
  if (!(p.back_lo <= p.back_hi)) return fail(RV_ERR_VALUE, me + ": back_lo > back_hi (or a NaN)");
  if (!(p.length_lo <= p.length_hi) || !(p.length_lo >= 0.0f)) return fail(RV_ERR_VALUE, me + ": length_lo > length_hi or length_lo < 0 (or a NaN)");
  return RV_OK;
}
static int pr_launch(rv_world* w, const rv_push_route_params& p, int s, int h, int t, float* d_actions, int32_t* d_status) {
  int rc = route_field(w); if (rc != RV_OK) return rc;
  PrArgs a;
  a.p = p; a.field = w->d_route; a.actions = d_actions; a.status = d_status; a.S = s; a.h = h; a.t = t;
  const long long waves = (long long)w->n * s;
  hipLaunchKernelGGL(k_push_proposals_route, dim3((unsigned)((waves + RV_HP_WAVES - 1) / RV_HP_WAVES)), dim3(64 * RV_HP_WAVES), 0, w->stream,
                     w->d_envs, w->n, w->d_cfg, a);
  HIPCHK(hipGetLastError());
  return RV_OK;
}
int rv_get_route_field(rv_world* w, uint8_t* d_out) {
  WCHK(w);
  int rc = route_cfg_check(w, "rv_get_route_field"); if (rc != RV_OK) return rc;
  NEED(d_out, "rv_get_route_field");
  rc = route_field(w); if (rc != RV_OK) return rc;
  HIPCHK(hipMemcpyAsync(d_out, w->d_route, RV_PR_CELLS, hipMemcpyDeviceToDevice, w->stream));
  return RV_OK;
}
int rv_policy_route_multi(rv_world* w, const rv_push_route_params* h_params, int32_t s, float* d_actions, int32_t* d_status) {
  WCHK(w);
  if (!h_params) return fail(RV_ERR_VALUE, "rv_policy_route_multi: null params");
  int rc = pr_check(w, *h_params, s, "rv_policy_route_multi"); if (rc != RV_OK) return rc;
  NEED(d_actions, "rv_policy_route_multi");
  if (!aligned_to(d_actions, 4) || !aligned_to(d_status, 4)) return fail(RV_ERR_VALUE, "rv_policy_route_multi: the buffers must be 4-byte aligned");
  return pr_launch(w, *h_params, s, 1, 0, d_actions, d_status);
}
int rv_plan_propose_route(rv_world* plan, rv_world* src, const rv_push_route_params* h_params, int32_t s, int32_t h,
                          float* d_actions, float* d_states, float* d_rewards, uint8_t* d_dones, int32_t* d_status) {
  return plan_propose_run(plan, src, h_params, s, h, d_actions, d_states, d_rewards, d_dones, d_status, "rv_plan_propose_route",
    [](const rv_push_route_params&) { return RV_OK; },
    pr_check,
    [=](rv_world* w, const rv_push_route_params& p, int h_, int t) { return pr_launch(w, p, 1, h_, t, d_actions, d_status); });
}
int rv_reward(rv_world* w, float* d_reward, uint8_t* d_done) { WCHK(w); SIMPLE_LAUNCH(k_reward, w->d_envs, w->n, d_reward, d_done); return RV_OK; }
int rv_get_episode_returns(rv_world* w, float* d) { WCHK(w); NEED(d, "rv_get_episode_returns"); SIMPLE_LAUNCH(k_returns, w->d_envs, w->n, d); return RV_OK; }
int rv_get_stats(rv_world* w, rv_macro_stats* h) {
  WCHK(w); NEED(h, "rv_get_stats");
  HIPCHK(hipMemcpyAsync(h, w->d_stats, sizeof(rv_macro_stats), hipMemcpyDeviceToHost, w->stream));
  int q_err = 0;
  if (w->q_used) HIPCHK(hipMemcpyAsync(&q_err, w->d_q + RV_Q_ERR, sizeof(int), hipMemcpyDeviceToHost, w->stream));
  HIPCHK(hipStreamSynchronize(w->stream));
  if (w->q_used && getenv("RV_QUEUE_DEBUG")) {      // (measurement aid: what every XCD's queue did in the last queued launch)
    int dbg[8 * RV_Q_NQ];
    HIPCHK(hipMemcpy(dbg, w->d_q + RV_Q_DBG(0), sizeof(dbg), hipMemcpyDeviceToHost));
    int t_max = 0;
    for (int x = 0; x < RV_Q_NQ; ++x) if (dbg[8 * x] > 0 && dbg[8 * x + 2] > t_max) t_max = dbg[8 * x + 2];
    for (int x = 0; x < RV_Q_NQ; ++x)      // (s_memrealtime: 100 MHz, one counter for the device; >> 4: units of 0.16 us)
      fprintf(stderr, "queue of XCD %d: %d workgroups, %d tasks, %d envs bound to it, %d times an env was kept, %d tasks taken from another XCD's queue, its last workgroup left %.2f ms before the last of all\n",
              x, dbg[8 * x + 4], dbg[8 * x], dbg[8 * x + 3], dbg[8 * x + 1], dbg[8 * x + 5], dbg[8 * x] > 0 ? (t_max - dbg[8 * x + 2]) * 16.0 / 100e6 * 1e3 : 0.0);
  }
  if (w->q_used) {
    w->q_used = false;
    // (rv_env_kernel.h: the hand-over of an env block between two tasks is asserted, never repaired)
    if (q_err) return fail(RV_ERR_STATE, "task queue: a block arrived with the wrong step / launch number, or a ring overflowed (code " + std::to_string(q_err) + ")");
  }
  return RV_OK;
}
int rv_last_kernel_ms(rv_world* w, float* h_ms) {
  WCHK(w); NEED(h_ms, "rv_last_kernel_ms");
  if (!w->timed) return fail(RV_ERR_STATE, "rv_last_kernel_ms: no env kernel launched yet");
  HIPCHK(hipEventSynchronize(w->ev1));
  HIPCHK(hipEventElapsedTime(h_ms, w->ev0, w->ev1));
  return RV_OK;
}

}  // extern "C"
