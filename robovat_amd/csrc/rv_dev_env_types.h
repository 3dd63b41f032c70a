// rv_dev_env_types.h -- the state layout of one env and the constants every layer of the env program shares:
// the profiling hooks (RV_STOP*, RV_PROF*, RV_PCNT), the manifold slot indices (RV_TIDX,
// RV_BBIDX, RV_AIDX), JTarget / LTarget (controllable_body.py:28-233), DevEnv (the persistent block in HBM, staged in
// LDS), Row, Scratch, Shared, Consts, and the small predicates on them (brk_*, body_on, body_movable, ...).
#pragma once
#include "../../include/rovat.h"
#include "rv_dev_collide.h"

namespace rv {

// profiling hook: leave the substep after phase group n, still advancing the step
// counter so that the control schedule (IK every 10 substeps) stays representative
#ifdef __HIP_DEVICE_COMPILE__
#define RV_STOP(n) if (K.stop_after == (n)) { if (threadIdx.x == 0) S.e.sim_steps++; __syncthreads(); return; }
#define RV_STOPL(n) if (K.stop_after == (n)) { if (threadIdx.x == 0) S.e.sim_steps++; __syncthreads(); return 0; }
#else
#define RV_STOP(n)
#define RV_STOPL(n)
#endif

// RV_PROFILE build only: lane 0 adds the shader-clock time since the last mark to slot i
#if defined(RV_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void g_shared_prof(int i, unsigned long long t);
__device__ __forceinline__ void g_shared_profg(int g, int i, unsigned long long t);
#define RV_PROF(i) { if (threadIdx.x == 0) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_shared_prof(i, t_); } }
// per-group marks inside the narrow phase: the first lane of 16-lane group g adds the time
// since ITS last mark to slot 12 + i (g = 0: table owners of bodies 0/2, g = 1: their arm owners)
#define RV_PROFG(i) { if ((int)threadIdx.x == 0) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); g_shared_profg(0, (i), t_); } }
#else
#define RV_PROF(i)
#define RV_PROFG(i)
#endif
// RV_PROFILE build only: event counts in slots 32..39
#if defined(RV_PROFILE) && defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void g_shared_cnt(int i, int n);
#define RV_PCNT(i, n) { if (threadIdx.x == 0) g_shared_cnt((i), (n)); }
#else
#define RV_PCNT(i, n)
#endif

#define RV_STEPS_TO_CHECK_DONE 100   // controllable_body.py:21
#define RV_STEPS_TO_UPDATE_IK  10    // controllable_body.py:24

#define RV_TIDX(b) (b)
#define RV_BBIDX(k) (RV_MAXB + (k))
#define RV_AIDX(b) (RV_MAXB + RV_NBB + (b))

// JointTarget / LinkTarget (controllable_body.py:28-233)
struct JTarget {
  int active, n_idx, has_vel, has_stop;
  int from_ik;   // the target is the IK solution of the active link target: 1 = yes, 2 = yes and the
                 // solve ended on the residual test (a re-solve from it returns it unchanged)
  int idx[RV_NJ];
  float pos[RV_NJ];
  float start_t, stop_t, pos_thr, vel_thr;
};
struct LTarget {
  int active, has_pose, nq, has_stop;
  float pose[7];
  float queue[RV_MAXQ][7];
  float start_t, stop_t, pos_thr, vel_thr;
};

// Persistent per-env state: one contiguous block in HBM, staged in LDS.
struct DevEnv {
  float body[RV_MAXB][RV_BODY_STRIDE];
  int active[RV_MAXB], frozen[RV_MAXB], shape[RV_MAXB];
  int asleep[RV_MAXB], sleep_count[RV_MAXB], deact_count[RV_MAXB];
  int still_count[RV_MAXB]; float still_ref[RV_MAXB][7];   // pose window of the in-place oscillation test
  int undisturbed[RV_MAXB];   // woken, but has not left the pose window it was sleeping in
  float baabb[RV_MAXB][6];   // world box (lo, hi) of the hulls + margin, taken when the body fell asleep
  float scale[RV_MAXB], mass[RV_MAXB], inv_mass[RV_MAXB], inv_inertia[RV_MAXB][3], friction[RV_MAXB], radius[RV_MAXB];
  // user constraint (Simulator.add_constraint, simulator.py:166-224; bullet_physics.py:748-957): a fixed
  // joint between the frame (con_lpos, con_lquat) of the body and a frame of the world (con_tpos,
  // con_tquat), which can apply at most con_fmax N per row
  int con_on[RV_MAXB]; float con_lpos[RV_MAXB][3], con_lquat[RV_MAXB][4], con_tpos[RV_MAXB][3], con_tquat[RV_MAXB][4], con_fmax[RV_MAXB];
  float table_z;
  // the camera this env is observed with: rv_config's calibration + the noise drawn at its last reset (ArmEnv._reset_camera,
  // arm_env.py:109-152): fx, fy, cx, cy, skew; rotation (row-major); translation
  float cam_intrinsics[5], cam_rotation[9], cam_translation[3];
  int n_bodies;
  int arm_enabled;
  float q[RV_NJ], qd[RV_NJ];
  int motor_on[RV_NJ];
  float motor_q[RV_NJ], motor_kp[RV_NJ], motor_kd[RV_NJ], vmax_cmd[RV_NJ];
  JTarget jt;
  LTarget lt;
  float gripper_ready_time;
  float fpos[RV_NFRAME][3], fquat[RV_NFRAME][4];
  DevMan man[RV_NMAN];
  int flag_arm_table, flag_arm_body[RV_MAXB];
  int sim_steps, num_steps, num_episodes, done, phase, is_safe, is_effective, reset_count, substeps_last, awake_last, pairs_last;
  int stepped;      // this env executed an env.step() in the last macro launch
  // rv_step_begin / rv_step_poll (partial batches): an env.step() that is spread over several
  // launches.  in_step: 0 no step pending, 1 stepping, 2 a step was begun on a finished episode
  // (reported as finished with reward 0, like rv_step_macro skips it); step_stage: -1 not started,
  // 0 in the phase loop, 1 in the closing wait_until_stable; ms_*: the locals of _execute_action
  // that have to survive the launch boundary
  int in_step, step_stage;
  int ms_num_waypoints, ms_interrupt, ms_has_budget, ms_max_phase_steps, ms_wus_steps, ms_wus_stable;
  float ms_wp[RV_MAXG][2][7], ms_start_pos[RV_MAXB][3], ms_start_yaw[RV_MAXB];
  int reward_valid; // last_reward is the reward of the env.step() the last rv_step_macro / rollout gave this env
                    // (set by the step, cleared when a macro launch skips the env or the env is reset; other launches leave it)
  float episode_reward, last_reward;
  float action[RV_MAXG][4];
  float obs_pos[RV_MAXB][3], prev_obs_pos[RV_MAXB][3];
  float obs_quat[RV_MAXB][4];   // ... and the orientations at that moment (the observation of an env.step() is taken before get_reward, robot_env.py:246-248)
  int num_total_steps, num_unsafe, num_ineffective, num_useful, num_successes;
  // env.attributes (push_env.py:368-375, 637-644): the counters the attribute observations
  // and the heuristic policy see are captured at the START of _execute_action / _reset_scene
  int obs_num_steps, obs_num_episodes;
  // per-launch sums for rv_get_stats (a rollout launch takes several steps per env)
  int l_unsafe, l_ineffective, l_useful, l_episodes, l_successes;
  // lateral friction of the finger tips / the table (Link.set_dynamics, grasp_4dof_env.py:262-293);
  // PushEnv leaves them at PHYSICS.ARM_FRICTION / SIM.TABLE.FRICTION
  float mu_finger, mu_table;
  int num_action_steps;       // Grasp4DofEnv: substeps spent in the 'start' phase
  // rollouts through the task queue (rv_env_kernel.h): how many tasks of the running launch this block has been through, and
  // the sum of its other words when it was last handed on -- the next workgroup takes the block only when both are right
  int q_seq; unsigned q_sum;
#ifdef RV_PROFILE
  unsigned long long prof[48], prof_t, prof_t2[4];   // tools/prof_rollout.py: shader-clock time per substep part
#endif
};
static_assert(sizeof(DevEnv) % 4 == 0, "DevEnv is copied word-wise");

// one solver row set per contact point (normal + two friction directions)
struct Row {
  float dir[3][3], rxa[3][3], rxb[3][3], aa[3][3], ab[3][3];
  float invk[3], vbc[3];
  float target, mu;
  // dynamic finger (rv_config.finger_dynamics): the row also acts on finger joint 7 + fidx with
  // Jacobian jf = -(dir . slide axis); fidx = -1: no finger involved
  float jf[3]; int fidx;
  float cap;   // largest normal impulse the row may carry (arm effort limit); 1e30: none
};

struct Scratch {
  float frot[RV_NFRAME][9], fv[RV_NFRAME][3], fw[RV_NFRAME][3], axis[RV_NLIMB][3];
  float colv[RV_NCOL][8][3], colc[RV_NCOL][3], colr[RV_NCOL];
  float colmin[RV_NCOL][3], colmax[RV_NCOL][3];   // world AABB of each collider box
  int arm_moving;
  int colflag[RV_NCOL];
  float rot[RV_MAXB][9], iinv[RV_MAXB][9];
  float tablev[8][3], groundv[8][3];
  // solver rows + world hull vertices (rebuilt before every use: the solver borrows them as
  // scratch for the velocity update)
  struct {
    struct {
#if !RV_ON_DEVICE
      Row rows[RV_NMAN][4];      // host emulation only: on the device every solver sets its rows up in registers
#endif
      float wv[RV_MAXB][RV_MAXH][RV_MAXV][3];
    } r;
  } u;
  // macro-step locals that must survive across phases
  float wp[RV_MAXG][2][7];
  float gstart[7];                       // Grasp4DofEnv: the grasp pose of this step
  float start_pos[RV_MAXB][3], start_yaw[RV_MAXB];
  float poses[RV_MAXB][7];
  int num_waypoints, interrupt, has_budget, max_phase_steps;
  int loop_break, wus_steps, wus_stable, valid;
  int wake[RV_MAXB];                     // wake test -> body-velocity phase (host emulation; the device keeps a mask in an SGPR)
  // budget of the running sim_run (rv_step_poll): at most bud_sub substeps / bud_clk shader
  // clocks from bud_t0 in this launch (0 = no limit); suspended: the call returned on the budget
  int bud_sub, bud_sub0, suspended, wus_resume;
  unsigned long long bud_clk, bud_t0;
  int ready[RV_MAXB];                    // the body's own deactivation tests say it may sleep (islands sleep as a whole)
  float res[16];
  float mot[RV_MAXB];
  float sync;
  // ControllableBody._update_ik as a wave-wide solve: seed / solution, Jacobian, flags
  float ik_q[RV_NLIMB], ik_J[6][RV_NLIMB]; int ik_need, ik_conv;
  float lq[RV_NLIMB][4];
  float vdraw[RV_NJ], ratio[RV_NJ];      // motor phase: raw commanded velocity, limit factor (host emulation; registers on the device)
  float fing_dv[2], fing_vt[2], fing_qd0[2];   // finger motors this substep: velocity step taken, commanded velocity, velocity after it
  // limb dynamics (rv_config.limb_dynamics): the same of the limb joints; centres of mass, joint-space
  // inertia, the Gauss-Jordan workspace [M | 1] -> [. | M^-1], generalised gravity force, motor-row bounds
  // and targets; per arm contact row (12 x body + 3 x point + direction) the joint-space Jacobian,
  // M^-1 Ja^T and the effective mass
  float limb_dv[RV_NLIMB], limb_vt[RV_NLIMB], limb_qd0[RV_NLIMB];
  float lcom[RV_NLIMB + 1][3], lA[RV_NLIMB][2 * RV_NLIMB], lGq[RV_NLIMB];
  float llo[RV_NLIMB], lhi[RV_NLIMB], ltgt[RV_NLIMB];
  // (rows 0..11: the arm rows of the ONE awake body the lane-per-row solver handles; the last seven: the motor rows,
  // e_j and column j of M^-1.  The one-lane system solver, which takes the cases with several awake bodies, derives
  // the rows of a point when it visits it: limb_point_row)
  float lJa[12 + RV_NLIMB][RV_NLIMB], lMiJ[12 + RV_NLIMB][RV_NLIMB], linvk[12];
  int jmoving[RV_NJ], jchg[RV_NJ];       // joint moves / changed at all in this substep (host emulation; JointMasks on the device)
  float rvec[RV_NLIMB + 1][3];           // FK: link offsets rotated into the world
  int jt_applied;                        // the motor targets hold the current joint target (per launch)
  int atflag[RV_NCOL];                   // collider box may be within the contact-query distance of the table
  int kin_fresh;                         // FK / collider scratch matches the joint state (per launch)
  // "arm far" substeps (sim_substep_light): joint path lengths since the collider boxes were last computed, whether
  // those boxes exist at all in this launch, substeps taken far since then, and this substep's verdict
  float ftravel[RV_NJ]; int far_valid, far_n, far;
  int nearf[RV_MAXB][RV_NCOL], bnear[RV_MAXB], near_any;   // wake test stage 1 -> stage 2 (host emulation; ballots on the device)
  float sep[RV_MAXB][RV_NCOL], coltravel[RV_NCOL];          // distance-bound culling of the wake queries
  float cdelta[3][RV_NCOL];                                 // coasting: box travel bound per candidate length
  float clr_t[RV_NCOL], clr_b[RV_NCOL]; int clr_valid;      // coasting: clearances left (table, bodies)
  float jtravel[RV_NJ];                                     // coasting: joint path lengths of the chunk
  float ccoef[RV_NCOL][RV_NJ];                              // coasting: lever of joint j on collider box col (col_travelled's weights)
  float crun[RV_NCOL][RV_NJ];                               // ... as measured on the last fresh kinematics (coast_measure_clearances)
  int fused_n, fused_pending;
  int coast_unsafe[3];
  float jlen[RV_NLIMB + 1], colext[RV_NCOL];   // |jpos_i|; collider extent from its frame origin
  float fext[RV_NFRAME], fmot[RV_NFRAME];     // per frame: largest collider extent; vertex travel this substep
  int any_on;
  int pairs[4];
  // narrow-phase work list (per substep): refreshed distances / break flags per cached point,
  // (body, collider box) proximity flags, the owners that have convex queries to run.  The queries are dealt to the
  // 16-lane groups by convex PAIR: the items (owner, pair) form one flat list in owner order, then pair order;
  // olist[k] = owner + 256 x the index of its first item, n_items = the length of the flat list
  // (ow_run: host emulation only, the owner's pair count before its far collider boxes are dropped)
  float rf_dist[RV_NMAN * 4]; int rf_rm[RV_NMAN * 4];
  int cn[RV_MAXB][RV_NCOL];
  int ow_run[RV_NMAN + RV_NCOL], olist[RV_NMAN + RV_NCOL], n_olist, n_items;
  QStage qst[4];                         // what the queries of the running round found, one slot per group
  int wvneed[RV_MAXB];                   // body has hulls in a convex query of this substep (host emulation; the device keeps
                                         // the mask in an SGPR and never touches these 16 B: the next LDS word wanted can replace them)
#if !RV_ON_DEVICE
  int rowmap[120], n_rows;   // host emulation of the impulse-space solver: rows in visiting order
#endif
  Rng rng;
};

struct Shared {
  DevEnv e;
  Scratch s;
  // launch constants staged in LDS: a pointer argument is not provably wave-uniform, so reading
  // rv_config / rv_arm through it would be a vector global load (L2 latency) per field
  rv_config cfg;
  rv_arm arm;
  int n_hulls[RV_MAXB];
  int n_verts[RV_MAXB][RV_MAXH];
};

struct Consts {
  const rv_config* cfg;     // LDS copy (Shared::cfg) inside kernels
  const rv_arm* arm;        // LDS copy (Shared::arm) inside kernels
  const rv_scene* scene;    // global memory: hull vertices / inertia only
  int stop_after;
};

RV_DEV int bb_a(int k) { return k < 3 ? 0 : (k < 5 ? 1 : 2); }
RV_DEV int bb_b(int k) { return k == 0 ? 1 : (k == 1 ? 2 : (k == 2 ? 3 : (k == 3 ? 2 : 3))); }
// round-robin colouring: round r solves pairs {r, 5-r}, which touch disjoint bodies
RV_DEV int bb_round_pair(int r, int x) { return x == 0 ? r : 5 - r; }

// Contact-breaking threshold of a manifold = rv_config.breaking x the smaller "angular motion disc" of
// the two shapes (btCollisionShape::getContactBreakingThreshold, btPersistentManifold): the disc of a
// movable is its bounding radius about the body origin, that of a collider box its half diagonal;
// the table's and the ground's are larger than any of them.
RV_DEV float brk_body(const DevEnv& e, const rv_config* c, int b) { return c->breaking * (e.radius[b] - c->margin); }
RV_DEV float brk_col(const rv_arm* arm, const rv_config* c, int col) {
  const float* h = arm->col_half[col];
  return c->breaking * fsqrtr(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
}
RV_DEV float brk_bb(const DevEnv& e, const rv_config* c, int a, int b) { return fminr(brk_body(e, c, a), brk_body(e, c, b)); }
RV_DEV float brk_ab(const DevEnv& e, const rv_arm* arm, const rv_config* c, int a, int col) { return fminr(brk_body(e, c, a), brk_col(arm, c, col)); }
// kind: 0 body-table, 1 body-body, 2 arm-body (col = the collider box)
RV_DEV float brk_of(const DevEnv& e, const rv_arm* arm, const rv_config* c, int kind, int a, int b, int col) {
  return kind == 0 ? brk_body(e, c, a) : (kind == 1 ? brk_bb(e, c, a, b) : brk_ab(e, arm, c, a, col));
}
// how close a moving collider box must come to the hulls of a sleeping body to wake it
RV_DEV float wake_range(const DevEnv& e, const rv_arm* arm, const rv_config* c, int b, int col) { return fminr(brk_ab(e, arm, c, b, col), c->wake_gap); }
RV_DEV float sim_time(const Shared& S, const Consts& K) { return K.cfg->dt * (float)S.e.sim_steps; }
RV_DEV int body_present(const DevEnv& e, int b) { return e.active[b] && !e.frozen[b]; }
RV_DEV int body_on(const DevEnv& e, int b) { return e.active[b] && !e.frozen[b] && !e.asleep[b]; }
// A STATIC body (Simulator.add_body(..., is_static=True), simulator.py:195-224; the wall of ArmEnv._reset_scene,
// arm_env.py:94-99): mass 0 as in Bullet -- inverse mass and inverse inertia 0.  It keeps its slot and its pair manifolds
// with the other bodies (their rows see a party that no impulse moves); it has no manifold with the table or the arm, takes
// no gravity and is not integrated; the arm does not wake it.  The env logic (observations, reward, safety, policies) looks
// at MOVABLE bodies only.
RV_DEV int body_static(const DevEnv& e, int b) { return e.inv_mass[b] == 0.0f; }
RV_DEV int body_movable(const DevEnv& e, int b) { return e.active[b] && !body_static(e, b); }
// start of a launch: nothing stepped yet (one lane)
RV_DEV void launch_counters_zero(DevEnv& e) {
  e.substeps_last = 0; e.awake_last = 0; e.pairs_last = 0; e.stepped = 0;
  e.l_unsafe = 0; e.l_ineffective = 0; e.l_useful = 0; e.l_episodes = 0; e.l_successes = 0;
}

}  // namespace rv
